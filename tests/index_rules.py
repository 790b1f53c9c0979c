"""numpy restatements of the reference's CumSum (src/ops/reduce.rs:217-257), GatherElements (src/ops/gather.rs:196-284), Trilu (src/ops/trilu.rs:15-64)
and Tile (src/ops/concat.rs:239-272): the rules the kernels of rten_amd/csrc/scan.hip and the host evaluation of include/rten_hip_graph.hpp are held to,
bit for bit.  Errors are (kind, message) of the reference's OpError.

cum_sum is the reference's loop written out -- NOT np.cumsum: the accumulator starts at +0 and the first add is `+0.0 + x0`, so a leading -0.0 gives +0.0
(np.cumsum copies the first element and keeps -0.0); every partial sum is one rounded float32 add, in walking order; int32 wraps."""
import numpy as np

F = np.float32


class RuleError(Exception):
    def __init__(self, kind, msg):
        super().__init__(f"{kind}({msg!r})")
        self.kind, self.msg = kind, msg


def resolve_axis(nd, axis):
    if axis < -nd or axis >= nd:
        raise RuleError("InvalidValue", "Axis is invalid")
    return axis + nd if axis < 0 else axis


def cum_sum(x, axis, exclusive=False, reverse=False):
    x = np.asarray(x)
    assert x.dtype in (np.dtype(F), np.dtype(np.int32))
    ax = resolve_axis(x.ndim, axis)
    lanes = np.moveaxis(x, ax, 0)                    # [axis_len, ...]: one step of the loop handles every lane at once, the order inside a lane is the loop's
    out = np.empty_like(lanes)
    acc = np.zeros(lanes.shape[1:], x.dtype)         # +0.0 / 0
    order = range(lanes.shape[0] - 1, -1, -1) if reverse else range(lanes.shape[0])
    with np.errstate(over="ignore", invalid="ignore"):
        for t in order:
            prev = acc
            if x.dtype == np.dtype(np.int32):
                acc = ((np.asarray(acc, np.int64) + np.asarray(lanes[t], np.int64)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)  # wraps
            else:
                acc = (acc + lanes[t]).astype(F)     # one rounded float32 add
            out[t] = prev if exclusive else acc
    return np.ascontiguousarray(np.moveaxis(out, 0, ax))


def chunked_sum(x, chunk):
    """What a scan that sums WITHIN chunks and then adds the chunk totals would give for a 1-D float32 lane (inclusive, forward): the reassociation
    the kernels must not do.  Used by the tests to show that their inputs can tell the two orders apart."""
    x = np.asarray(x, F)
    out = np.empty_like(x)
    carry = F(0)
    for c0 in range(0, x.size, chunk):
        local = cum_sum(x[c0:c0 + chunk], 0)
        out[c0:c0 + chunk] = (carry + local).astype(F)
        carry = out[min(c0 + chunk, x.size) - 1]
    return out


def gather_elements(x, indices, axis=0, clamp=False):
    """`clamp`: the device's deliberate deviation -- an out-of-range index reads the nearest end of the axis instead of being an error."""
    x, indices = np.asarray(x), np.asarray(indices)
    if x.ndim != indices.ndim:
        raise RuleError("IncompatibleInputShapes", "Input and indices must have same rank")
    ax = resolve_axis(x.ndim, axis)
    for d in range(x.ndim):
        if d != ax and indices.shape[d] > x.shape[d]:
            raise RuleError("IncompatibleInputShapes", "`indices` size must be <= input size in non-axis dimensions")
    alen = x.shape[ax]
    idx = indices.astype(np.int64)
    idx = np.where(idx < 0, idx + alen, idx)
    if indices.size and (alen == 0 or ((idx < 0) | (idx >= alen)).any()):
        if not clamp or alen == 0:
            raise RuleError("InvalidValue", "Entry in `indices` is out of range")
        idx = np.clip(idx, 0, alen - 1)
    trimmed = x[tuple(slice(None) if d == ax else slice(0, indices.shape[d]) for d in range(x.ndim))]
    if indices.size == 0:
        return np.zeros(indices.shape, x.dtype)
    return np.ascontiguousarray(np.take_along_axis(trimmed, idx, ax))


def trilu(x, k=0, upper=True):
    x = np.asarray(x)
    if x.ndim < 2:
        raise RuleError("InvalidValue", "Input must have >= 2 dims")
    rows, cols = x.shape[-2:]
    delta = np.arange(rows, dtype=np.int64)[:, None] + int(k) - np.arange(cols, dtype=np.int64)[None, :]
    keep = delta <= 0 if upper else delta >= 0
    out = np.zeros_like(x)                            # the all-zero word: +0.0 / 0 (np.where, not a multiplication: a masked NaN does not survive)
    np.copyto(out, x, where=np.broadcast_to(keep, x.shape))
    return out


def tile(x, repeats):
    x = np.asarray(x)
    repeats = [int(r) for r in np.asarray(repeats).reshape(-1)]
    if len(repeats) != x.ndim or any(r < 0 for r in repeats):
        raise RuleError("InvalidValue", "invalid repeats")
    return np.ascontiguousarray(np.tile(x, repeats)) if x.ndim else x.copy()
