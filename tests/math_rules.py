"""Expected values for Pad, Pow, the unary math operators, PRelu and the variadic Min / Max / Sum / Mean, restated in numpy.

Exactly rounded operators (src/ops/unary_elementwise.rs, variadic_elementwise.rs, binary_elementwise.rs:977-987): every function here is one IEEE
float32 operation per step, so its bits are the reference's bits.
  sign   Rust signum: +0 -> 1, -0 -> -1, NaN -> NaN (not ONNX's 0).
  round  round_ties_even.
  exp    rten-vecmath's polynomial = the oracle's ref.exp.
  vmin / vmax   a left fold of cmp_nan_less / cmp_nan_greater (reduce.rs:847-873): a NaN in either operand wins, a tie keeps the left operand.
  mean   the sum divided by n as f32 (a division, not a multiplication by the reciprocal).
  pow    exponent 2 -> x * x, 3 -> x * x * x (two roundings), tested per element.

Operators the reference hands to the host's libm (Log = ln, Pow's general case = powf, Softplus = exp(x).ln_1p()): "the reference's bits" are not
defined there.  The contract is the float64 function rounded once to float32; softplus rounds exp(x) to float32 first, as the reference does, so
x >= 88.73 gives +inf.  The float64 functions are libm's, called one element at a time (numpy's own vector loops may take a different routine).
tests/test_math_pad_ops.py checks that these rules are within one ulp of the host's float32 libm with equal special values.

pad: src/ops/pad.rs, including what rem_euclid does when a reflect pad is >= the axis length."""
import ctypes as C

import numpy as np

F = np.float32
_LIBM = C.CDLL("libm.so.6")


class RuleError(Exception):
    """kind = the OpError variant, msg = its text."""

    def __init__(self, kind, msg):
        super().__init__(f"{kind}({msg!r})")
        self.kind, self.msg = kind, msg


def _libm64(name, nargs=1):
    fn = getattr(_LIBM, name)
    fn.restype, fn.argtypes = C.c_double, [C.c_double] * nargs
    return fn


def _map64(name, *arrays):
    """float32 operands -> libm's float64 `name` per element -> rounded once to float32."""
    fn = _libm64(name, len(arrays))
    arrays = np.broadcast_arrays(*[np.asarray(a, np.float32) for a in arrays])
    out = np.empty(arrays[0].shape, np.float64)
    flat = [a.ravel() for a in arrays]
    o = out.reshape(-1)
    for i in range(o.size):
        o[i] = fn(*[float(a[i]) for a in flat])
    with np.errstate(all="ignore"):
        return out.astype(np.float32)


def _f(x):
    return np.asarray(x, np.float32)


# ------------------------------------------------------------------------------------------------ unary
def neg(x):
    x = np.asarray(x)
    if x.dtype == np.int32:
        return (np.uint32(0) - x.view(np.uint32)).view(np.int32)  # wrapping: i32::MIN stays
    return (_f(x).view(np.uint32) ^ np.uint32(0x80000000)).view(np.float32)


def abs_(x):
    x = np.asarray(x)
    if x.dtype == np.int32:
        return np.where(x < 0, neg(x), x).astype(np.int32)
    return (_f(x).view(np.uint32) & np.uint32(0x7fffffff)).view(np.float32)


def sign(x):
    x = np.asarray(x)
    if x.dtype == np.int32:
        return ((x > 0).astype(np.int32) - (x < 0).astype(np.int32)).astype(np.int32)
    x = _f(x)
    return np.where(np.isnan(x), F(np.nan), np.copysign(F(1), x)).astype(np.float32)


def floor(x):
    return np.floor(_f(x))


def ceil(x):
    return np.ceil(_f(x))


def round_(x):
    return np.rint(_f(x))  # ties to even; -0.4 -> -0.0


def sqrt(x):
    with np.errstate(all="ignore"):
        return np.sqrt(_f(x))


def reciprocal(x):
    with np.errstate(all="ignore"):
        return (F(1) / _f(x)).astype(np.float32)


def exp(x):
    from oracle import ref
    return ref.exp(np.ascontiguousarray(_f(x)))


def log(x):
    return _map64("log", x)


def softplus(x):
    return _map64("log1p", _map64("exp", x))


UNARY = {"Neg": neg, "Abs": abs_, "Sign": sign, "Floor": floor, "Ceil": ceil, "Round": round_, "Sqrt": sqrt, "Reciprocal": reciprocal, "Exp": exp,
         "Log": log, "Softplus": softplus}


# ------------------------------------------------------------------------------------------------ binary / variadic
def _broadcast(a, b):
    try:
        return np.broadcast_arrays(a, b)
    except ValueError:
        raise RuleError("IncompatibleInputShapes", "Cannot broadcast inputs")


def min2(a, b):
    a, b = _broadcast(np.asarray(a), np.asarray(b))
    if a.dtype == np.int32:
        return np.where(a <= b, a, b).astype(np.int32)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(a <= b, a, b))).astype(np.float32)


def max2(a, b):
    a, b = _broadcast(np.asarray(a), np.asarray(b))
    if a.dtype == np.int32:
        return np.where(a >= b, a, b).astype(np.int32)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(a >= b, a, b))).astype(np.float32)


def add2(a, b):
    a, b = _broadcast(np.asarray(a), np.asarray(b))
    if a.dtype == np.int32:
        return (a.view(np.uint32) + b.view(np.uint32)).view(np.int32)  # wrapping
    with np.errstate(all="ignore"):
        return (a + b).astype(np.float32)


def _fold(inputs, f2):
    """reduce_elementwise (variadic_elementwise.rs:21-39): one input is a copy, otherwise a left fold."""
    if not inputs:
        raise RuleError("InvalidValue", "Expected at least one input")
    acc = np.array(inputs[0], copy=True)
    for b in inputs[1:]:
        acc = f2(acc, np.asarray(b))
    return acc


def vmin(*inputs):
    return _fold(inputs, min2)


def vmax(*inputs):
    return _fold(inputs, max2)


def vsum(*inputs):
    return _fold(inputs, add2)


def mean(*inputs):
    s = vsum(*[_f(i) for i in inputs])
    with np.errstate(all="ignore"):
        return (s / F(len(inputs))).astype(np.float32)


def pow_(base, exponent):
    b, e = _broadcast(_f(base), _f(exponent))
    with np.errstate(all="ignore"):
        sq = (b * b).astype(np.float32)
        cube = (sq * b).astype(np.float32)
    general = _map64("pow", b, e)
    return np.where(e == F(2), sq, np.where(e == F(3), cube, general)).astype(np.float32)


def prelu(x, slope):
    x, slope = _f(x), _f(slope)
    try:
        s = np.broadcast_to(slope, x.shape)
    except ValueError:
        raise RuleError("IncompatibleInputShapes", "Slope is not broadcastable to input shape")
    with np.errstate(all="ignore"):
        return np.where(x < F(0), (s * x).astype(np.float32), x).astype(np.float32)


# ------------------------------------------------------------------------------------------------ Pad
def src_index(mode, o, length, p):
    """ReflectPad / EdgePad / WrapPad::src_index (pad.rs:235-286) for an array of output coordinates."""
    o = np.asarray(o, np.int64)
    if mode == "reflect":
        s = np.where(o < p, p - o, np.where(o < length + p, o - p, length - (o - length - p) - 2))
        return np.mod(s, length)  # rem_euclid
    if mode == "edge":
        return np.clip(o - p, 0, length - 1)
    if mode == "wrap":
        return np.mod(o - p, length)
    raise ValueError(mode)


def pad(x, pads, mode="constant", value=0, axes=None):
    x = np.asarray(x)
    pads = [int(p) for p in np.asarray(pads).reshape(-1)]
    nd = x.ndim
    if axes is not None:
        raise RuleError("UnsupportedValue", "Pad operator does not yet support `axes` input")
    if len(pads) != 2 * nd:
        raise RuleError("InvalidValue", "padding length should be 2 * input dims")
    if any(p < 0 for p in pads):
        region = []
        for d in range(nd):
            cb, ce = max(-pads[d], 0), max(-pads[nd + d], 0)
            if cb + ce > x.shape[d]:
                raise RuleError("InvalidValue", "Negative pads remove more elements than axis contains")
            region.append(slice(cb, x.shape[d] - ce))
        x = x[tuple(region)]
    pb = [max(pads[d], 0) for d in range(nd)]
    out_shape = tuple(pb[d] + x.shape[d] + max(pads[nd + d], 0) for d in range(nd))
    if out_shape == x.shape:
        return np.array(x, copy=True)
    if mode == "constant":
        y = np.full(out_shape, value, x.dtype)
        y[tuple(slice(pb[d], pb[d] + x.shape[d]) for d in range(nd))] = x
        return y
    batch = max(nd - 2, 0)
    if out_shape[:batch] != x.shape[:batch]:
        raise RuleError("UnsupportedValue", "Pad only supports non-constant padding of last 2 dims")
    if 0 in x.shape[batch:]:
        raise RuleError("InvalidValue", "Padded dimension for non-constant padding is empty")
    idx = [np.arange(out_shape[d]) if d < batch else src_index(mode, np.arange(out_shape[d]), x.shape[d], pb[d]) for d in range(nd)]
    return np.ascontiguousarray(x[np.ix_(*idx)])


# ------------------------------------------------------------------------------------------------ comparison helpers
def ulp_distance(a, b):
    """Distance in float32 steps between two arrays, on the ordered-integer line (+0 and -0 coincide); NaN against NaN is 0, NaN against a number is huge."""
    a, b = _f(a), _f(b)

    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(b))
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    return np.where(both_nan, 0, np.where(one_nan, 1 << 40, d))


def same_bits(a, b):
    """Bitwise equality, with any NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | nan).all())
