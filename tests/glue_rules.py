"""The reference's semantics of the glue operators, restated in numpy: Shape, Slice, Concat, Expand, Where, ConstantOfShape, NonZero, Range, Cast,
Not / And / Or / Xor, the comparisons, integer and float Add / Sub / Mul / Div, Gather, Transpose and the view operators.

One plain function per operator, written from the reference's source with its fast paths (the citation is on each function).  Every function moves
values or applies one IEEE / two's-complement operation per step, so its bits are the reference's bits; tests/golden/glue_reference.json pins the
functions to the literals of the reference's own unit tests (tests/test_glue_ops.py).  Errors are RuleError(kind, message) with the reference's strings.

Element types: float32, int32, uint8, int8.  ONNX int64 and bool are int32 from load on (onnx_loader.rs:332-339: int64 saturates, bool is 0 / 1).

Where the reference has no defined value this file says so and pins what the backend does, identically on its host and its device path:
  i32::MIN / -1     Rust panics (overflow).  Pinned: i32::MIN (the wrapping quotient), `idiv`.
  Range, int32      `val + delta` past i32::MAX panics in a debug build and wraps in a release build.  Pinned: wrapping.
and where a kernel cannot report what the reference reports, the DEVICE value is a function of its own:
  idiv_device       a zero in a divisor that only the device knows gives 0 for that element (the reference: InvalidValue "Divisor contains zero")
  gather_device     an out-of-range index on device data is clamped into the axis (the reference: InvalidValue "Entry in `indices` is out of range")
"""
import numpy as np

from tests.math_rules import RuleError

F, I32, U8, I8 = np.float32, np.int32, np.uint8, np.int8
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _c(a):
    """A C-contiguous copy that keeps a 0-d array 0-d (np.ascontiguousarray gives shape [1])."""
    return np.array(a, order="C")


def same_bits(a, b):
    """Equal dtype, shape and bytes (NaN payloads and the sign of zero included)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and _c(a).tobytes() == _c(b).tobytes()


def sat32(v):
    """int64 -> int32 as the loader narrows an initializer (onnx_loader.rs:464-492): saturating."""
    return np.clip(np.asarray(v, np.int64), I32_MIN, I32_MAX).astype(I32)


def wrap32(v):
    """The low 32 bits of an int64 result as int32: Rust's wrapping_* / release-build overflow."""
    return (np.asarray(v, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(I32).reshape(np.shape(v))


def resolve_axis(ndim, axis):
    """src/ops/mod.rs resolve_axis"""
    a = axis + ndim if axis < 0 else axis
    if a < 0 or a >= ndim:
        raise RuleError("InvalidValue", "Axis is invalid")
    return a


def broadcast_shape(*shapes):
    """rten-tensor broadcast_shapes; binary_elementwise.rs:263, 1196-1198 for the message"""
    nd = max(len(s) for s in shapes)
    out = [1] * nd
    for s in shapes:
        for i, d in enumerate(s):
            o = nd - len(s) + i
            if d != 1:
                if out[o] != 1 and out[o] != d:
                    raise RuleError("IncompatibleInputShapes", "Cannot broadcast inputs")
                out[o] = d
    return tuple(out)


def _bcast(*arrays):
    shape = broadcast_shape(*[a.shape for a in arrays])
    return [np.broadcast_to(a, shape) for a in arrays]


# ------------------------------------------------------------------------------------------------ Shape
def shape(x_shape, start=None, end=None):
    """src/ops/layout.rs:475-505 with Shape::resolve_start_end (rten-shape-inference/src/ops/layout.rs:251-276): negative values count from the end, both are clamped to [0, rank]."""
    nd = len(x_shape)
    s = 0 if start is None else (start + nd if start < 0 else start)
    e = nd if end is None else (end + nd if end < 0 else end)
    s, e = min(max(s, 0), nd), min(max(e, 0), nd)
    return np.array(list(x_shape[s:e]) if e > s else [], I32)


# ------------------------------------------------------------------------------------------------ Slice
def slice_ranges(x_shape, starts, ends, axes=None, steps=None):
    """src/ops/slice.rs:29-85 and SliceRange::clamp / steps (rten-tensor/src/slice_range.rs:235-288).  starts / ends / axes / steps are int32 in the
    reference (an int64 operand saturates at load).  Forward: indices are clamped to [-len, len]; backward: to [-len - 1, len - 1]; a negative index
    then counts from the end.  Returns (first index, count, step) per axis of x."""
    nd = len(x_shape)
    starts, ends = [int(v) for v in sat32(starts)], [int(v) for v in sat32(ends)]
    axes = None if axes is None else [int(v) for v in sat32(axes)]
    steps = None if steps is None else [int(v) for v in sat32(steps)]
    if axes is not None and len(axes) > nd:
        raise RuleError("InvalidValue", "`axes` length must be <= input rank")
    n_axes = nd if axes is None else len(axes)
    if len(starts) != n_axes:
        raise RuleError("InvalidValue", "`starts` length must match axis count")
    if len(ends) != n_axes:
        raise RuleError("InvalidValue", "`ends` length must match axis count")
    if steps is not None:
        if len(steps) != n_axes:
            raise RuleError("InvalidValue", "`steps` length must match axis count")
        if any(s == 0 for s in steps):
            raise RuleError("InvalidValue", "steps must be non-zero")
    out = [(0, int(d), 1) for d in x_shape]
    for i, (st, en) in enumerate(zip(starts, ends)):
        ax = resolve_axis(nd, axes[i]) if axes is not None else i
        step = 1 if steps is None else steps[i]
        n = int(x_shape[ax])
        lo, hi = (-n, n) if step > 0 else (-n - 1, n - 1)
        st, en = min(max(st, lo), hi), min(max(en, lo), hi)
        st, en = (st if st >= 0 else n + st), (en if en >= 0 else n + en)
        if step > 0:
            count = 0 if en <= st else 1 + (en - st - 1) // step
        else:
            count = 0 if en >= st else 1 + (st - en - 1) // -step
        out[ax] = (st, count, step)
    return out


def slice(x, starts, ends, axes=None, steps=None):  # noqa: A001 (the operator's name)
    """The input form (opset >= 10).  Elements are moved, never computed: -0.0 and NaN payloads keep their bits."""
    x = np.asarray(x)
    idx = []
    for st, count, step in slice_ranges(x.shape, starts, ends, axes, steps):
        idx.append(np.arange(count, dtype=np.int64) * step + st)
    return _c(x[np.ix_(*idx)]) if x.ndim else x.copy()


def slice_attrs(x, starts, ends, axes=None):
    """The opset-1 form: starts / ends / axes as attributes, step 1 (the reference's loader turns them into the inputs above)."""
    return slice(x, starts, ends, axes)


# ------------------------------------------------------------------------------------------------ Concat, Expand, Where
def concat(xs, axis):
    """src/ops/concat.rs:21-108.  The first input fixes the rank and the other extents."""
    xs = [np.asarray(x) for x in xs]
    ax = resolve_axis(xs[0].ndim, axis)
    for x in xs:
        if x.ndim != xs[0].ndim:
            raise RuleError("IncompatibleInputShapes", "Tensors must have the same number of dimensions")
        if any(d != ax and x.shape[d] != xs[0].shape[d] for d in range(x.ndim)):
            raise RuleError("IncompatibleInputShapes", "Dimensions must be the same except for concat axis")
    return np.concatenate(xs, axis=ax)


def expand(x, target):
    """src/ops/layout.rs:106-118, 177-262: numpy broadcasting of x against the VALUES of `target` (a 1 in the target keeps x's extent)."""
    x = np.asarray(x)
    target = [int(v) for v in sat32(target)]
    if any(d < 0 for d in target):
        raise RuleError("InvalidValue", "Target shape contains negative values")
    try:
        out = broadcast_shape(x.shape, tuple(target))
    except RuleError:
        raise RuleError("IncompatibleInputShapes", "Cannot broadcast input with target shape") from None
    return _c(np.broadcast_to(x, out))


def where(cond, x, y):
    """binary_elementwise.rs:1189-1280: cond != 0 ? x : y over the three-way broadcast; the chosen element is moved (payload bits survive)."""
    cond, x, y = np.asarray(cond, I32), np.asarray(x), np.asarray(y)
    c, xb, yb = _bcast(cond, x, y)
    words = np.where(c != 0, _c(xb).view(np.uint32), _c(yb).view(np.uint32))
    return _c(words.astype(np.uint32)).view(x.dtype).reshape(c.shape)


# ------------------------------------------------------------------------------------------------ ConstantOfShape, NonZero, Range
def constant_of_shape(shape_values, value=None):
    """src/ops/generate.rs:18-64.  `value`: None (the default, float32 0), or a numpy scalar of float32 / int32 / int64 / bool; int64 saturates
    to int32 like every int64 tensor the loader reads, bool is int32 0 / 1."""
    if value is None:
        fill = F(0)
    else:
        v = np.asarray(value)
        fill = F(v) if v.dtype == F else (I32(v != 0) if v.dtype == np.bool_ else sat32(v)[()])
    dims = [int(v) for v in sat32(shape_values)]
    if any(d < 0 for d in dims):
        raise RuleError("InvalidValue", "Invalid shape")
    return np.full(dims, fill, fill.dtype)


def nonzero(x):
    """src/ops/reduce.rs:299-325: int32 [rank, count], the indices of the elements != 0 in row-major order.  -0.0 == 0 (not listed), NaN != 0
    (listed).  A rank-0 input gives shape [0, 0 or 1]."""
    x = np.asarray(x)
    if x.ndim == 0:
        return np.zeros((0, 1 if x != 0 else 0), I32)
    with np.errstate(invalid="ignore"):
        return _c(np.argwhere(x != 0).T.astype(I32).reshape(x.ndim, -1))


def range_(start, limit, delta):
    """src/ops/generate.rs:170-189: push val, then val = val + delta, while val has not reached `limit` -- an accumulation in the element type, so a
    float32 range carries the accumulated roundings and its COUNT follows from them (not ceil((limit - start) / delta))."""
    t = np.asarray(start).dtype.type
    assert t in (F, I32)
    if delta == 0:
        raise RuleError("InvalidValue", "delta must be non-zero")
    out = []
    if t is F:
        val, limit, delta = F(start), F(limit), F(delta)
        while (delta > 0 and val < limit) or (delta < 0 and val > limit):
            out.append(val)
            val = F(val + delta)
        return np.array(out, F)
    val, limit, delta = int(start), int(limit), int(delta)
    while (delta > 0 and val < limit) or (delta < 0 and val > limit):
        out.append(val)
        val = int(wrap32(val + delta))
    return np.array(out, I32)


# ------------------------------------------------------------------------------------------------ Cast
_INT_BOUNDS = {I32: (I32_MIN, I32_MAX), U8: (0, 255), I8: (-128, 127)}


def cast(x, to):
    """src/ops/convert.rs:18-62: Rust `as` for every pair of float32 / int32 / uint8 / int8.  float -> int truncates toward zero, saturates at the
    target's bounds, NaN -> 0; int -> narrower int keeps the low bits; int -> float32 rounds to nearest even; same type copies."""
    x = np.asarray(x)
    to = np.dtype(to).type
    if x.dtype.type is to:
        return x.copy()
    if x.dtype.type is F and to is not F:
        lo, hi = _INT_BOUNDS[to]
        v = x.astype(np.float64)
        with np.errstate(invalid="ignore"):
            v = np.where(np.isnan(v), 0.0, np.clip(np.trunc(v), lo, hi))
        return v.astype(np.int64).astype(to)
    if to is F:
        return x.astype(F)  # (exact below 2^24; int32 beyond it rounds to nearest even, as numpy and the hardware conversion do)
    return (x.astype(np.int64) & ((1 << (8 * np.dtype(to).itemsize)) - 1)).astype(np.dtype(to).str.replace("i", "u")).view(to)


# ------------------------------------------------------------------------------------------------ logic and comparisons
def logical_not(x):
    """unary_elementwise.rs:563-565: int32 x == 0"""
    return (np.asarray(x, I32) == 0).astype(I32)


def logical(op, a, b):
    """binary_elementwise.rs:546-598: operands are true when != 0; int32 0 / 1"""
    a, b = _bcast(np.asarray(a, I32) != 0, np.asarray(b, I32) != 0)
    return {"And": a & b, "Or": a | b, "Xor": a ^ b}[op].astype(I32)


def compare(op, a, b):
    """binary_elementwise.rs:733-786 on two float32 or two int32 operands: IEEE comparisons (any comparison with a NaN is false; +0 == -0)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.dtype.type in (F, I32)
    a, b = _bcast(a, b)
    with np.errstate(invalid="ignore"):
        r = {"Equal": np.equal, "Less": np.less, "LessOrEqual": np.less_equal, "Greater": np.greater, "GreaterOrEqual": np.greater_equal}[op](a, b)
    return r.astype(I32)


# ------------------------------------------------------------------------------------------------ arithmetic
def iarith(op, a, b):
    """binary_elementwise.rs:476-495, 891, 1130 on int32: wrapping Add / Sub / Mul (a release build)."""
    a, b = _bcast(np.asarray(a, I32).astype(np.int64), np.asarray(b, I32).astype(np.int64))
    return wrap32({"Add": a + b, "Sub": a - b, "Mul": a * b}[op])


def idiv(a, b):
    """binary_elementwise.rs:604-637 on int32: a zero ANYWHERE in the divisor is InvalidValue("Divisor contains zero"), checked before anything is
    computed (check_nonzero); the quotient truncates toward zero.  i32::MIN / -1 is a panic in Rust: pinned to i32::MIN."""
    a, b = np.asarray(a, I32), np.asarray(b, I32)
    if (b == 0).any():
        raise RuleError("InvalidValue", "Divisor contains zero")
    a64, b64 = _bcast(a.astype(np.int64), b.astype(np.int64))
    q = np.abs(a64) // np.abs(b64)
    return wrap32(np.where((a64 < 0) != (b64 < 0), -q, q))


def idiv_device(a, b):
    """The element-wise kernel on a divisor only the device knows (a graph input): x / 0 = 0 for that element, no error (docs/KERNELS.md)."""
    a, b = np.asarray(a, I32), np.asarray(b, I32)
    safe = np.where(b == 0, 1, b).astype(I32)
    return np.where(np.broadcast_to(b, broadcast_shape(a.shape, b.shape)) == 0, 0, idiv(a, safe)).astype(I32)


def farith(op, a, b):
    """binary_elementwise.rs:476-495, 891, 1130 on float32: one IEEE operation per element."""
    a, b = _bcast(np.asarray(a, F), np.asarray(b, F))
    with np.errstate(all="ignore"):
        return {"Add": np.add, "Sub": np.subtract, "Mul": np.multiply}[op](a, b).astype(F)


def div_f32(a, b):
    """binary_elementwise.rs:613-637 (div) and :640-661 (div_in_place): when `b.item()` is Some -- the divisor holds exactly ONE element, at any rank
    -- the result is a * (1 / b): the reciprocal rounded to float32, then one multiplication.  Every other divisor is a true division.  The rule
    looks at the RIGHT operand only: a one-element dividend divides."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all="ignore"):
        if b.size == 1:
            r = (F(1) / b).astype(F)
            x, y = _bcast(a, r)
            return np.multiply(x, y).astype(F)
        x, y = _bcast(a, b)
        return np.divide(x, y).astype(F)


# ------------------------------------------------------------------------------------------------ Gather
def gather(x, ids, axis=0):
    """src/ops/gather.rs:60-160 (numpy.take): negative indices count from the end; an index outside [-len, len) is
    InvalidValue("Entry in `indices` is out of range"), also when the axis is empty and there is an index."""
    x, ids = np.asarray(x), np.asarray(ids, I32)
    ax = resolve_axis(x.ndim, axis)
    n = x.shape[ax]
    idx = ids.astype(np.int64)
    idx = np.where(idx < 0, idx + n, idx)
    if ((idx < 0) | (idx >= n)).any():
        raise RuleError("InvalidValue", "Entry in `indices` is out of range")
    return _c(np.take(x, idx, axis=ax))


def gather_device(x, ids, axis=0):
    """The device kernels on indices only the device knows: after the negative wrap, an index is clamped into [0, len - 1] (include/rten_hip.h)."""
    x, ids = np.asarray(x), np.asarray(ids, I32)
    ax = resolve_axis(x.ndim, axis)
    n = x.shape[ax]
    idx = ids.astype(np.int64)
    idx = np.clip(np.where(idx < 0, idx + n, idx), 0, n - 1)
    return _c(np.take(x, idx, axis=ax))


# ------------------------------------------------------------------------------------------------ Transpose and the views
def transpose(x, perm=None):
    """src/ops/layout.rs:647-670: perm absent reverses the axes; a perm that is not a permutation of the axes is refused."""
    x = np.asarray(x)
    if perm is None:
        return _c(x.transpose())
    p = [a + x.ndim if a < 0 else a for a in perm]
    if sorted(p) != list(range(x.ndim)):
        raise RuleError("InvalidValue", "Permutation is invalid")
    return _c(x.transpose(p))


def squeeze(x, axes=None):
    """src/ops/layout.rs:560-600"""
    x = np.asarray(x)
    if axes is None:
        return x.reshape([d for d in x.shape if d != 1])
    ax = sorted(resolve_axis(x.ndim, int(a)) for a in axes)
    if any(x.shape[a] != 1 for a in ax):
        raise RuleError("InvalidValue", "Can only remove dimensions of size 1")
    return x.reshape([d for i, d in enumerate(x.shape) if i not in ax])


def unsqueeze(x, axes):
    """src/ops/layout.rs:710-745: the axes index the OUTPUT"""
    x = np.asarray(x)
    nd = x.ndim + len(axes)
    ax = sorted(resolve_axis(nd, int(a)) for a in axes)
    if len(set(ax)) != len(ax):
        raise RuleError("InvalidValue", "Axes must be unique")
    shape_, src = [], iter(x.shape)
    for i in range(nd):
        shape_.append(1 if i in ax else next(src))
    return x.reshape(shape_)


def reshape(x, target, allow_zero=False):
    """src/ops/layout.rs:324-391 (resolve_shape), its checks in its order: 0 copies the input's extent (unless allow_zero), one -1 is inferred"""
    x = np.asarray(x)
    target = [int(v) for v in sat32(target)]
    infer, known = None, 1
    for i, d in enumerate(target):
        if d < -1:
            raise RuleError("InvalidValue", "Invalid dimension size in shape")
        if d == 0 and not allow_zero:
            if i >= x.ndim:
                raise RuleError("InvalidValue", "Zero dim has no corresponding input dim")
            known *= x.shape[i]
        elif d != -1:
            known *= d
        elif infer is not None:
            raise RuleError("InvalidValue", "Multiple dimensions in new shape set to -1")
        else:
            infer = i
    if infer is not None:
        if known == 0:
            raise RuleError("InvalidValue", "Cannot infer size of -1 dim when other dims are zero")
        if x.size % known:
            raise RuleError("InvalidValue", "Input length does not match target shape")
    elif known != x.size:
        raise RuleError("InvalidValue", "Input length does not match target shape")
    return x.reshape([x.size // known if d == -1 else (x.shape[i] if d == 0 and not allow_zero else d) for i, d in enumerate(target)])


def flatten(x, axis=1):
    """src/ops/layout.rs:231-250 (flattened_shape): [prod(shape[:axis]), prod(shape[axis:])]; axis may equal the rank"""
    x = np.asarray(x)
    a = axis + x.ndim if axis < 0 else axis
    if a < 0 or a > x.ndim:
        raise RuleError("InvalidValue", "Axis is invalid")
    return x.reshape(int(np.prod(x.shape[:a], dtype=np.int64)), int(np.prod(x.shape[a:], dtype=np.int64)))
