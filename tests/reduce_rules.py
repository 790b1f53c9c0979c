"""Expected values for ReduceL1 / ReduceSumSquare / ReduceL2 / ReduceLogSum / ReduceLogSumExp / ReduceProd, LpNormalization and GlobalMaxPool, restated on
the CPU oracle (the expectations of tests/test_reduce_ops.py and tests/test_gpu_reduce_family.py).  Written from the reference (src/ops/reduce.rs:414-520,
590-845, 1046-1100, 1167-1234, rten-vecmath/src/sum.rs:37-159, rten-simd/src/iter.rs:70-120, src/ops/norm.rs:611-650, src/ops/pooling.rs:477-553), not from
the device code.

  * Sum is the oracle's (oracle.einsum.reduce_sum: fold_unroll<4> over 16-lane vectors, lanes added from lane 0).
  * SumAbs is that Sum of |x|: taking |x| is exact, so `acc + |x|` has the bits of adding the element |x|.
  * SumSquare is restated slot by slot: the same walk with acc = fmaf(x, x, acc), a correctly rounded float32 fused multiply-add from libm (a float64
    x * x + acc rounded to float32 is rounded twice and is NOT the same thing); the four accumulators merge, and the 16 lanes add up, by plain adds.
  * SumExpSub is a plain fold: ONE 16-lane accumulator, element i added into lane i % 16 in order, exp = the oracle's full-range Exp (ref.exp).
  * ln is norm_rules.correctly_rounded_ln: the float64 logarithm rounded once to float32 (ln 0 = -inf, ln of a negative number = NaN).
  * Prod is a left fold from 1.
  * int32 arithmetic wraps in two's complement (|i32::MIN| = i32::MIN).
"""
import ctypes as C

import numpy as np

from oracle import einsum as oe
from oracle import ref
from tests import norm_rules

F = np.float32
LANES = 16
KINDS = ("l1", "sum_square", "l2", "log_sum", "log_sum_exp", "prod")
INT32_KINDS = ("l1", "sum_square", "prod")

_LIBM = C.CDLL("libm.so.6")
_LIBM.fmaf.restype = C.c_float
_LIBM.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]


class RuleError(Exception):
    """kind = the OpError variant, msg = its text."""

    def __init__(self, kind, msg=""):
        super().__init__(f"{kind}({msg!r})")
        self.kind, self.msg = kind, msg


def fmaf(a, b, c):
    return F(_LIBM.fmaf(float(a), float(b), float(c)))


def ln(s):
    s = F(s)
    if np.isnan(s) or s < 0:
        return F(np.nan)
    if s == 0:
        return F(-np.inf)
    return norm_rules.correctly_rounded_ln(s)


def fold_unroll4(xs, fold):
    """rten-simd/src/iter.rs:97-120 over 16-lane vectors: four accumulators while 64 elements remain, merged by plain adds, then whole vectors and the
    masked tail folded into the merged accumulator, then the lanes added from lane 0."""
    xs = np.asarray(xs, np.float32)
    n, i = xs.size, 0
    acc = [[F(0)] * LANES for _ in range(4)]
    with np.errstate(all="ignore"):
        while n - i >= 4 * LANES:
            for u in range(4):
                for l in range(LANES):
                    acc[u][l] = fold(acc[u][l], xs[i + LANES * u + l])
            i += 4 * LANES
        a = acc[0]
        for u in range(1, 4):
            a = [F(a[l] + acc[u][l]) for l in range(LANES)]
        while n - i >= LANES:
            a = [fold(a[l], xs[i + l]) for l in range(LANES)]
            i += LANES
        for l in range(n - i):  # masked tail: the other lanes keep their value
            a[l] = fold(a[l], xs[i + l])
        s = F(0)
        for l in range(LANES):
            s = F(s + a[l])
    return s


def sum_square(xs):
    return fold_unroll4(xs, lambda acc, x: fmaf(x, x, acc))


def sum_abs(xs):
    return F(oe.reduce_sum(np.abs(np.asarray(xs, np.float32)).reshape(-1), [0])) if np.size(xs) else F(0)


def vec_sum(xs):
    return F(oe.reduce_sum(np.asarray(xs, np.float32).reshape(-1), [0])) if np.size(xs) else F(0)


def max_num(xs):
    """vecmath::MaxNum: a NaN anywhere gives NaN; an empty slice gives -inf."""
    xs = np.asarray(xs, np.float32)
    if np.isnan(xs).any():
        return F(np.nan)
    return F(xs.max()) if xs.size else F(-np.inf)


def sum_exp_sub(xs, m):
    xs = np.asarray(xs, np.float32)
    with np.errstate(all="ignore"):
        e = ref.exp((xs - F(m)).astype(np.float32))
        acc = [F(0)] * LANES
        for i in range(xs.size):
            acc[i % LANES] = F(acc[i % LANES] + e[i])
        s = F(0)
        for l in range(LANES):
            s = F(s + acc[l])
    return s


def log_sum_exp(xs):
    m = max_num(xs)
    if not np.isfinite(m):
        return m
    with np.errstate(all="ignore"):
        return F(m + ln(sum_exp_sub(xs, m)))


def prod(xs):
    p = F(1)
    with np.errstate(all="ignore"):
        for x in np.asarray(xs, np.float32):
            p = F(p * x)
    return p


def _sqrt(s):
    with np.errstate(all="ignore"):
        return F(np.sqrt(F(s)))


SLICE_F32 = {
    "l1": sum_abs,
    "sum_square": sum_square,
    "l2": lambda xs: _sqrt(sum_square(xs)),
    "log_sum": lambda xs: ln(vec_sum(xs)),
    "log_sum_exp": log_sum_exp,
    "prod": prod,
}


def _wrap(v):
    return np.int32(np.uint32(int(v) & 0xFFFFFFFF))


def _slice_i32(kind, xs):
    vals = [int(v) for v in np.asarray(xs, np.int32)]
    if kind == "l1":
        return _wrap(sum(int(_wrap(-v)) if v < 0 else v for v in vals))
    if kind == "sum_square":
        return _wrap(sum(v * v for v in vals))
    p = 1
    for v in vals:
        p = int(_wrap(p * v))
    return _wrap(p)


def resolve_axes(nd, axes):
    out = []
    for a in axes:
        a = int(a)
        if a < -nd or a >= nd:
            raise RuleError("InvalidValue", "Axis is invalid")
        out.append(a + nd if a < 0 else a)
    return sorted(set(out))


def noop_value(kind, x):
    """noop_with_empty_axes with no axes (reduce.rs:627-629,690-694,755-759,828-830,1082-1084,1216-1218): the reduction is skipped, the operator's element
    map is not."""
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        if kind == "l1":
            return np.abs(x) if x.dtype.kind == "f" else np.array([_wrap(-int(v)) if v < 0 else v for v in x.reshape(-1)], np.int32).reshape(x.shape)
        if kind == "sum_square":
            return (x * x).astype(np.float32) if x.dtype.kind == "f" else np.array([_wrap(int(v) * int(v)) for v in x.reshape(-1)], np.int32).reshape(x.shape)
        if kind == "log_sum":
            return np.array([ln(v) for v in x.reshape(-1)], np.float32).reshape(x.shape)
    return x.copy()


def check_type(kind, x, noop=False):
    """The reference's refusals: L2 is float32 only behind map_value_view! (UnsupportedType, after the noop test); LogSum / LogSumExp take their input through
    require_as::<f32> (a cast error, before it); L1 / SumSquare / Prod take float32 and int32."""
    k = np.asarray(x).dtype
    if k == np.float32 or (k == np.int32 and kind in INT32_KINDS):
        return
    if kind in ("log_sum", "log_sum_exp"):
        raise RuleError("InputCastFailed", "expected float32 tensor")
    if noop and kind in ("l2", "prod"):
        return
    raise RuleError("UnsupportedType")


def reduce(kind, x, axes=None, keepdims=True, noop_with_empty_axes=False):
    """reduce(), reduce.rs:414-520: resolved axes sorted and unique; a slice = the reduced dims walked row-major in their original relative order; a 0-d
    input is a slice of one element; an empty slice gives the kernel's value for it."""
    x = np.asarray(x)
    none = axes is None or len(axes) == 0
    check_type(kind, x, noop=none and noop_with_empty_axes)
    if none and noop_with_empty_axes:
        return noop_value(kind, x)
    f = SLICE_F32[kind] if x.dtype == np.float32 else (lambda xs: _slice_i32(kind, xs))
    if x.ndim == 0:
        if not none:
            resolve_axes(0, axes)
        return np.asarray(f(x.reshape(1)), x.dtype)
    ax = resolve_axes(x.ndim, axes) if not none else list(range(x.ndim))
    keep = [d for d in range(x.ndim) if d not in ax]
    kshape = tuple(x.shape[d] for d in keep)
    rshape = tuple(x.shape[d] for d in ax)
    xp = np.transpose(x, keep + ax)
    nrows = int(np.prod(kshape, dtype=np.int64))
    nred = int(np.prod(rshape, dtype=np.int64))
    rows = np.ascontiguousarray(xp).reshape(nrows, nred) if x.size else np.zeros((nrows, 0), x.dtype)
    out = np.empty(nrows, x.dtype)
    for r in range(nrows):
        out[r] = f(rows[r])
    return out.reshape([1 if d in ax else x.shape[d] for d in range(x.ndim)]) if keepdims else out.reshape(kshape)


def lp_normalization(x, axis=-1, p=2):
    """lp_normalization, norm.rs:611-650: per lane along `axis`, norm = SumAbs (p = 1) or sqrt(SumSquare) (p = 2); a zero norm zeroes the lane; otherwise
    x * (1 / norm) -- one division, one multiply per element."""
    x = np.asarray(x, np.float32)
    if p not in (1, 2):
        raise RuleError("UnsupportedValue", "`p` must be 1 or 2")
    if axis < -x.ndim or axis >= x.ndim:
        raise RuleError("InvalidValue", "Axis is invalid")
    if x.shape[axis] == 0 or x.size == 0:
        return x.copy()
    t = np.ascontiguousarray(np.moveaxis(x, axis, -1))
    rows = t.reshape(-1, t.shape[-1])
    y = np.empty_like(rows)
    with np.errstate(all="ignore"):
        for r in range(rows.shape[0]):
            norm = sum_abs(rows[r]) if p == 1 else _sqrt(sum_square(rows[r]))
            y[r] = 0 if norm == 0 else (rows[r] * F(F(1) / norm)).astype(np.float32)
    return np.ascontiguousarray(np.moveaxis(y.reshape(t.shape), -1, axis))


def global_max_pool(x):
    """global_max_pool, pooling.rs:477-514,549-553: MaxNum over dims 2.. of an input of at least 2 dims; output [N, C, 1, ...]."""
    x = np.asarray(x, np.float32)
    if x.ndim < 2:
        raise RuleError("InvalidValue", "Input must have at least 2 dims")
    n, c = x.shape[:2]
    rows = x.reshape(n * c, -1)
    out = np.array([max_num(rows[r]) for r in range(n * c)], np.float32)
    return out.reshape((n, c) + (1,) * (x.ndim - 2))


def pairwise_prod(xs):
    """A tree product (what a parallel reduction would compute): the test rows of ReduceProd must tell it from the left fold."""
    xs = [F(v) for v in np.asarray(xs, np.float32)]
    with np.errstate(all="ignore"):
        while len(xs) > 1:
            xs = [F(xs[i] * xs[i + 1]) if i + 1 < len(xs) else xs[i] for i in range(0, len(xs), 2)]
    return xs[0] if xs else F(1)


def canon(a):
    """Bit patterns for an exact comparison, every NaN mapped to one NaN."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a.astype(np.int32).view(np.uint32)
    b = a.astype(np.float32).view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    g, w = canon(got), canon(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} differ, first at {i}: got {got[i]!r} ({g[i]:#010x}) want {want[i]!r} ({w[i]:#010x})")
