"""The selection family's rules restated with numpy (the expected values of tests/test_select_ops.py and tests/test_gpu_select_ops.py).

Written from the behaviour of the reference (src/ops/reduce.rs:64-215, 876-1044, 1236-1356), not from the device code: comparisons are ordinary
floating-point / integer comparisons on the values, never bit tricks.

  * reduce_minmax: extreme of each slice; a NaN anywhere in the slice gives NaN; an empty slice gives the identity.  The sign of a zero extreme and the
    payload of a NaN are not part of the contract (compare through `canon`).
  * arg_minmax: Iterator::max_by with cmp_nan_greater -- the FIRST NaN of a lane that holds one (ArgMin too), otherwise the LAST element equal to the extreme.
  * topk: NaN is greater than every number whatever `largest` says; larger (or smaller) values first; equal values by ascending index; several NaNs by
    ascending index (the device's definition; the reference's comparator is inconsistent there).
"""
import numpy as np


class RuleError(Exception):
    """An OpError::InvalidValue of the reference, by its message."""


IDENT = {("max", "f"): -np.inf, ("min", "f"): np.inf, ("max", "i"): np.iinfo(np.int32).min, ("min", "i"): np.iinfo(np.int32).max}


def resolve_axis(nd, axis):
    if axis < -nd or axis >= nd:
        raise RuleError("Axis is invalid")
    return axis + nd if axis < 0 else axis


def reduce_minmax(x, axes=None, keepdims=True, op="max", noop_with_empty_axes=False):
    x = np.asarray(x)
    if (axes is None or len(axes) == 0) and noop_with_empty_axes:
        return x.copy()
    if x.ndim == 0:
        for a in (axes if axes is not None else []):
            resolve_axis(0, a)
        return x.copy()
    ax = tuple(sorted({resolve_axis(x.ndim, int(a)) for a in axes})) if axes is not None and len(axes) else tuple(range(x.ndim))
    fn = np.max if op == "max" else np.min
    with np.errstate(invalid="ignore"):
        y = fn(x, axis=ax, keepdims=keepdims, initial=x.dtype.type(IDENT[(op, x.dtype.kind)]))  # numpy's max / min propagate NaN, like maximum_num / minimum_num
    return np.asarray(y, x.dtype)


def arg_minmax(x, axis=0, keepdims=True, op="max"):
    x = np.asarray(x)
    ax = resolve_axis(x.ndim, axis)
    n = x.shape[ax]
    if n == 0:
        raise RuleError("Cannot select index from empty sequence")
    xm = np.moveaxis(x, ax, -1)
    if xm.size == 0:
        out = np.zeros(xm.shape[:-1], np.int32)
    else:
        nan = np.isnan(xm) if x.dtype.kind == "f" else np.zeros(xm.shape, bool)
        first_nan = np.argmax(nan, axis=-1)
        with np.errstate(invalid="ignore"):
            ext = (np.max if op == "max" else np.min)(xm, axis=-1, keepdims=True)
        eq = xm == ext  # +0 == -0; all False on a lane with a NaN (not used there)
        last_eq = n - 1 - np.argmax(eq[..., ::-1], axis=-1)
        out = np.where(nan.any(axis=-1), first_nan, last_eq).astype(np.int32)
    return np.expand_dims(out, ax) if keepdims else out


def topk(x, k, axis=-1, largest=True):
    """(values, int32 indices), sorted."""
    x = np.asarray(x)
    if k < 0:
        raise RuleError("k must be positive")
    ax = resolve_axis(x.ndim, -1 if axis is None else axis)
    n = x.shape[ax]
    if k > n and k != 0:
        raise RuleError("k > dimension size")
    xm = np.moveaxis(x, ax, -1)
    nan = np.isnan(xm) if x.dtype.kind == "f" else np.zeros(xm.shape, bool)
    v = np.where(nan, 0, xm).astype(np.float64)  # exact for float32 and int32; -0.0 == 0.0 in the sort, as in partial_cmp
    idx = np.broadcast_to(np.arange(n), xm.shape)
    # np.lexsort: the LAST key is the primary one; all ascending
    order = np.lexsort((idx, -v, ~nan), axis=-1) if largest else np.lexsort((idx, v, nan), axis=-1)
    order = order[..., :k]
    vals = np.take_along_axis(xm, order, axis=-1)
    return np.ascontiguousarray(np.moveaxis(vals, -1, ax)), np.ascontiguousarray(np.moveaxis(order.astype(np.int32), -1, ax))


def canon(a, fold_zero_sign=False):
    """Bit patterns for an exact comparison: every NaN mapped to one NaN; with fold_zero_sign (ReduceMax / ReduceMin only) -0 mapped to +0."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a.astype(np.int32).view(np.uint32)
    b = a.astype(np.float32).view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    if fold_zero_sign:
        b[b == 0x80000000] = 0
    return b
