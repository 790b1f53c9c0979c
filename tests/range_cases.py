"""Operand bands at the ends of the f32 range, and the cases built on them, shared by tests/test_range_cases.py (CPU: every band's condition
on the oracle's output) and tests/test_gpu_range.py (device: the same inputs, the same expected bits).

Every other GPU suite draws its operands from rng.f32() - 0.5, where nothing underflows, overflows or absorbs a small addend.  The bands here
put finite operands near either end.  A band is a recipe AND a condition on what the oracle computes from it: a `tiny` case whose outputs were
ordinary numbers would pass on a kernel that flushes subnormals, so the condition (at least half the outputs are nonzero subnormals) is what
makes the case a test.  test_range_cases.py asserts the condition of every case below; the GPU file runs exactly these cases.

  band     recipe (A, B = the two multiplied operands; extra = bias / residual / C)              condition on the oracle's output
  tiny     A, B in 2^[-72,-66]; extra in 2^[-140,-128]                                          >= 50 % nonzero subnormals
  sub_a    A in 2^[-149,-127] (every element subnormal); B, extra in 2^[0,20]                   >= 90 % finite, normal, nonzero
  sub_b    the roles swapped                                                                    same
  huge     A in 2^[54,63]; B's even columns in 2^[54,62], odd columns in 2^[54,64]              finite >= 10 %, +-inf >= 10 %, NaN >= 1 %
  spread   A, B, extra in 2^[-40,40]                                                            all finite, normal (absorption: the order of the adds)

Conditions are checked on the value BEFORE a fused activation (Relu zeroes half of any sign-symmetric output, whatever its magnitude); the
activation itself is an element-wise map of that value.  The operator-specific bands (attention, softmax, the norms, RNN, MatMulNBits,
DynamicQuantizeLinear) are stated with their builders."""
import functools
import zlib

import numpy as np

from oracle import ref
from tests import norm_rules, rnn_rules

F = np.float32
TINY = float(np.finfo(np.float32).tiny)  # 2^-126, the smallest normal

BANDS = {
    "tiny": dict(a=(-72, -66), b=(-72, -66), extra=(-140, -128)),
    "sub_a": dict(a=(-149, -127), b=(0, 20), extra=(0, 20)),
    "sub_b": dict(a=(0, 20), b=(-149, -127), extra=(0, 20)),
    "huge": dict(a=(54, 63), b=(54, 62), b_odd=(54, 64), extra=(54, 63)),
    "spread": dict(a=(-40, 40), b=(-40, 40), extra=(-40, 40)),
}
MATRIX_BANDS = ("tiny", "sub_a", "sub_b", "huge", "spread")


def wide(rng, shape, lo, hi):
    """+-[1, 2) * 2^e, e uniform over the integers lo..hi, as float32 (below 2^-126 the mantissa is rounded to the subnormal grid: never to zero)."""
    n = int(np.prod(shape, dtype=np.int64))
    e = rng.integers(lo, hi + 1, n)
    m = (1.0 + rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return np.ldexp(m, e).astype(F).reshape(shape)


def operand(rng, band, role, shape):
    """Operand `role` ("a", "b" or "extra") of a band.  `huge` B: the columns (last axis) alternate between two exponent ranges, so that one output
    holds finite sums, overflowed sums and inf - inf."""
    spec = BANDS[band]
    if role == "b" and "b_odd" in spec:
        out = wide(rng, shape, *spec["b"])
        odd = wide(rng, shape, *spec["b_odd"])
        out[..., 1::2] = odd[..., 1::2]
        return out
    return wide(rng, shape, *spec[role])


def shares(y):
    """Fractions of a float32 tensor that are zero / nonzero subnormal / finite normal / infinite / NaN."""
    y = np.asarray(y, F).ravel()
    a = np.abs(y)
    n = max(y.size, 1)
    return dict(zero=float((a == 0).sum()) / n, sub=float(((a > 0) & (a < TINY)).sum()) / n, normal=float((np.isfinite(y) & (a >= TINY)).sum()) / n,
                inf=float(np.isinf(y).sum()) / n, nan=float(np.isnan(y).sum()) / n)


def all_subnormal(x):
    a = np.abs(np.asarray(x, F))
    return bool(((a > 0) & (a < TINY)).all())


def band_holds(band, y, one_block=False):
    """The band's condition on one oracle output -> (holds, shares).  `one_block`: the chain is a single depth block (K <= 256) of FMAs with nothing
    added behind it.  An FMA adds the EXACT product, which is finite for finite operands, so such a chain can reach +-inf but never inf - inf: NaN comes
    only from adding separately rounded parts (the fold between depth blocks, a residual that is itself inf).  `huge` then asks for finite and inf alone."""
    s = shares(y)
    if band == "tiny":
        ok = s["sub"] >= 0.5
    elif band in ("sub_a", "sub_b"):
        ok = s["normal"] >= 0.9
    elif band == "huge":
        ok = s["zero"] + s["sub"] + s["normal"] >= 0.1 and s["inf"] >= 0.1 and (one_block or s["nan"] >= 0.01)
    elif band == "spread":
        ok = s["normal"] == 1.0
    else:
        raise KeyError(band)
    return ok, s


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _quiet(fn):
    @functools.wraps(fn)
    def run(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    return run


# ------------------------------------------------------------------------------------------ GEMM
GEMM_SHAPE = (70, 300, 130)    # crosses the 256-deep block (the fold between depth blocks runs), a 12-wide k tail, ragged in 64- and 128-wide tiles
SMALLM_SHAPE = (16, 600, 40)   # variant 31: three depth blocks parked, then folded
ONE_ROW_SHAPE = (1, 530, 40)   # the one-row order, both B layouts
DENSE_SHAPE = (72, 300, 132)   # M and N multiples of 4: with A stored m-major the 16-byte loaders run, and each variant its own kernel on a dense B; as ragged as GEMM_SHAPE


@functools.lru_cache(maxsize=None)
@_quiet
def gemm_case(band, shape):
    """a, b, c, column bias; `plain` = a b; `pre` = .5 a b + 2 c + bias (then Relu / Gelu).  For one row the oracle follows the operand's layout
    (the reference's vector-matrix kernels), so `plain_bt` / `pre_bt` are the results for a transposed-storage B."""
    m, k, n = shape
    rng = _rng("gemm", band, shape)
    a, b = operand(rng, band, "a", (m, k)), operand(rng, band, "b", (k, n))
    c, bias = operand(rng, band, "extra", (m, n)), operand(rng, band, "extra", (n,))
    bt = np.ascontiguousarray(b.T).T
    out = dict(a=a, b=b, bt=bt, c=c, bias=bias, cond={})
    for tag, bb in (("", b), ("_bt", bt)):
        out["plain" + tag] = ref.gemm_f32(a, bb)
        pre = ref.gemm_f32(a, bb, c=c, alpha=0.5, beta=2.0, bias=bias, bias_kind=ref.BIAS_PER_COL)
        out["pre" + tag], out["relu" + tag], out["gelu" + tag] = pre, ref.relu(pre), ref.gelu(pre)
        out["cond"]["plain" + tag] = out["plain" + tag]
        out["cond"]["pre" + tag] = pre
    return out


GEMM_CASES = [(band, shape) for shape in (GEMM_SHAPE, SMALLM_SHAPE, ONE_ROW_SHAPE, DENSE_SHAPE) for band in MATRIX_BANDS]


# ------------------------------------------------------------------------------------------ convolution
# name -> (N, C, H, W, O, kh, kw, pads, strides, groups), bands
CONV_GEOMS = {
    "patch": ((1, 40, 9, 9, 70, 3, 3, (1, 1, 1, 1), (1, 1), 1), MATRIX_BANDS),      # K = 360; 3x3 / stride 1 / padding 1: the patch kernel's form (variant 30 runs)
    "stem": ((1, 3, 33, 70, 24, 7, 7, (2, 3, 3, 2), (2, 2), 1), MATRIX_BANDS),       # variants 32 and 3
    # 8464 columns = 266 tiles of 64x64: one whole round of a 256-unit chip and a remainder, the smallest size at which the thin-tile tail plan (split mode 4)
    # engages; K = 72 keeps the oracle quick (one depth block)
    "rounds": ((1, 8, 92, 92, 70, 3, 3, (1, 1, 1, 1), (1, 1), 1), MATRIX_BANDS),
    # K = 288 = 9 * 32: two depth blocks and a whole number of the lean persistent kernel's k-tiles (split mode 6); 81 columns, four ragged 64x64 tiles
    "lean": ((1, 32, 9, 9, 70, 3, 3, (1, 1, 1, 1), (1, 1), 1), MATRIX_BANDS),
    "dw_9x8": ((2, 5, 9, 8, 5, 3, 3, (1, 1, 1, 1), (1, 1), 5), ("tiny", "sub_a")),   # depthwise; rows of whole 16-byte groups: the streaming kernel, ragged row groups
    "dw_9x7": ((2, 5, 9, 7, 5, 3, 3, (1, 1, 1, 1), (1, 1), 5), ("tiny", "sub_a")),   # depthwise; W % 4 != 0: the generic (four rows per thread) kernel
    "dw_6x8": ((1, 5, 6, 8, 5, 3, 3, (1, 1, 1, 1), (1, 1), 5), ("tiny", "sub_a")),   # depthwise streaming, aligned
}
CONV_CASES = [(name, band) for name, (_, bands) in CONV_GEOMS.items() for band in bands]


@functools.lru_cache(maxsize=None)
@_quiet
def conv_case(name, band):
    """w is operand A, x operand B (the implicit GEMM's roles).  `plain` = conv(x, w); `pre` = conv + bias + residual; `full` = Relu(pre)."""
    (N, Cc, H, W, O, kh, kw, pads, strides, groups), _ = CONV_GEOMS[name]
    rng = _rng("conv", name, band)
    w, x = operand(rng, band, "a", (O, Cc // groups, kh, kw)), operand(rng, band, "b", (N, Cc, H, W))
    kw_ = dict(pads=pads, strides=strides, groups=groups)
    plain = ref.conv2d_f32(x, w, None, **kw_)
    bias, res = operand(rng, band, "extra", (O,)), operand(rng, band, "extra", plain.shape)
    pre = ref.conv2d_f32(x, w, bias, residual=res, **kw_)
    full = ref.conv2d_f32(x, w, bias, residual=res, relu=True, **kw_)
    return dict(x=x, w=w, bias=bias, res=res, pads=pads, strides=strides, groups=groups, plain=plain, pre=pre, full=full, cond=dict(plain=plain, pre=pre),
                one_block=(Cc // groups) * kh * kw <= 256)


# ------------------------------------------------------------------------------------------ pair kernels (two pointwise convolutions in one launch)
PAIR_GEOM = (3, 64, 10, 6, 128, 128)   # N, C1, H, W, M1, M2: ragged column counts (60 pixels per image)
PAIR_BANDS = ("tiny", "spread", "huge")
# the second layer's weights: y1 re-enters the second product from LDS.  tiny: y1 is subnormal (asserted), the weights ordinary, so y2 is subnormal too
PAIR_W2 = {"tiny": (-8, -3), "spread": (-20, 20), "huge": (54, 63)}
PAIR_CASES = [(form, band) for form in ("pair", "shortcut") for band in PAIR_BANDS]


@functools.lru_cache(maxsize=None)
@_quiet
def pair_case(form, band):
    """pair: y1 = Relu(conv(x, w1) + b1 + r), y2 = Relu(conv(y1, w2) + b2).  shortcut: r = conv(xs, ws) + bs is computed in the same launch and M2 = 64."""
    N, C1, H, W, M1, M2 = PAIR_GEOM
    if form == "shortcut":
        M2 = 64
    rng = _rng("pair", form, band)
    x, w1 = operand(rng, band, "b", (N, C1, H, W)), operand(rng, band, "a", (M1, C1, 1, 1))
    w2 = wide(rng, (M2, M1, 1, 1), *PAIR_W2[band])
    b1, b2 = operand(rng, band, "extra", (M1,)), operand(rng, band, "extra", (M2,))
    out = dict(x=x, w1=w1, w2=w2, b1=b1, b2=b2)
    if form == "shortcut":
        out["xs"], out["ws"], out["bs"] = operand(rng, band, "b", (N, C1, H, W)), operand(rng, band, "a", (M1, C1, 1, 1)), operand(rng, band, "extra", (M1,))
        r = ref.conv2d_f32(out["xs"], out["ws"], out["bs"])
    else:
        r = out["r"] = operand(rng, band, "extra", (N, M1, H, W))
    pre1 = ref.conv2d_f32(x, w1, b1, residual=r)
    out["want1"] = ref.conv2d_f32(x, w1, b1, residual=r, relu=True)
    pre2 = ref.conv2d_f32(out["want1"], w2, b2)
    out["want2"] = ref.conv2d_f32(out["want1"], w2, b2, relu=True)
    out["cond"] = dict(pre1=pre1) if band == "huge" else dict(pre1=pre1, pre2=pre2)  # (huge: y1 already holds inf, so y2 is inf / NaN throughout)
    out["one_block"] = form == "pair"  # K = 64 and a finite residual; the shortcut's residual is a computed convolution that overflows itself
    return out


# ------------------------------------------------------------------------------------------ ConvTranspose
# N, C, H, W, O_g, kh, kw, pads, strides, dilations, groups, output_padding (both from test_conv_transpose)
CONVT_GEOMS = {
    "fused": (1, 4, 8, 8, 3, 4, 4, (1, 1, 1, 1), (2, 2), (1, 1), 1, (0, 0)),
    "col2im": (2, 6, 5, 7, 4, 3, 2, (1, 0, 2, 1), (2, 3), (1, 2), 2, (1, 0)),
}
CONVT_BANDS = ("tiny", "sub_a", "spread")
CONVT_CASES = [(name, band) for name in CONVT_GEOMS for band in CONVT_BANDS]


@functools.lru_cache(maxsize=None)
@_quiet
def convt_case(name, band):
    N, Cc, H, W, og, kh, kw, pads, strides, dil, groups, opad = CONVT_GEOMS[name]
    rng = _rng("convt", name, band)
    w, x = operand(rng, band, "a", (Cc, og, kh, kw)), operand(rng, band, "b", (N, Cc, H, W))
    bias = operand(rng, band, "extra", (og * groups,))
    plain = ref.conv_transpose2d_f32(x, w, None, pads, strides, dil, groups, opad)
    biased = ref.conv_transpose2d_f32(x, w, bias, pads, strides, dil, groups, opad)
    # strides and dilations leave outputs that no tap lands on (structural zeros): the unbiased condition is about the others
    landed = ref.conv_transpose2d_f32(np.ones_like(x), np.ones_like(w), None, pads, strides, dil, groups, opad) != 0
    return dict(x=x, w=w, bias=bias, geom=(pads, strides, dil, groups, opad), plain=plain, biased=biased, cond=dict(plain=plain[landed], biased=biased))


# ------------------------------------------------------------------------------------------ attention
# name -> (B, H, S, T, head size): the kernel the one-kernel path (2) takes there
SDPA_SHAPES = {"sdpa_fused16_kernel": (1, 2, 64, 128, 64), "sdpa_fused_kernel": (1, 2, 40, 100, 64), "sdpa_fused_general_kernel": (1, 1, 33, 300, 32)}
SDPA_BANDS = ("v_sub", "peaky", "overflow")
SDPA_CASES = [(kernel, band) for kernel in SDPA_SHAPES for band in SDPA_BANDS]


@functools.lru_cache(maxsize=None)
@_quiet
def sdpa_case(kernel, band):
    """v_sub: V in 2^[-149,-127] (>= 20 % subnormal outputs; the probabilities are an MFMA operand against it).  peaky: scores spread over +-100 and more
    (softmax of the scores: >= 20 % exact zeros, >= 1 subnormal probability).  overflow: Q, K in 2^[55,63], the scores are +-inf: rows are NaN, or 0 flushed.
    want[(masked, flush)] for no mask / a [B, 1, 1, T] mask of 0 and -inf."""
    B, H, S, T, hd = SDPA_SHAPES[kernel]
    rng = _rng("sdpa", kernel, band)
    u = lambda *s: (rng.random(s, dtype=F) - F(0.5))  # noqa: E731
    q, k, v = u(B, H, S, hd), u(B, H, T, hd), u(B, H, T, hd)
    if band == "v_sub":
        v = wide(rng, v.shape, -149, -127)
    elif band == "peaky":
        q, k = q * F(30), k * F(30)
    else:
        q, k = wide(rng, q.shape, 55, 63), wide(rng, k.shape, 55, 63)
    mask = np.where(rng.random((B, 1, 1, T)) > 0.3, 0.0, -np.inf).astype(F)
    scale = F(1.0) / np.sqrt(F(hd))
    want = {(masked, flush): ref.sdpa(q, k, v, mask=mask if masked else None, scale=scale, lanes=16, flush_nan=flush) for masked in (False, True) for flush in (False, True)}
    scores = np.stack([ref.gemm_f32(q[b, h], np.ascontiguousarray(k[b, h].T)) * scale for b in range(B) for h in range(H)])
    return dict(q=q, k=k, v=v, mask=mask, scale=float(scale), want=want, probs=ref.softmax(scores, lanes=16))


def sdpa_holds(band, case):
    if band == "v_sub":
        s = shares(case["want"][(False, False)])
        return s["sub"] >= 0.2, s
    if band == "peaky":
        s = shares(case["probs"])
        return s["zero"] >= 0.2 and s["sub"] > 0, s
    s, z = shares(case["want"][(False, False)]), shares(case["want"][(False, True)])
    return s["nan"] >= 0.9 and z["zero"] >= 0.9, dict(unflushed=s, flushed=z)


# ------------------------------------------------------------------------------------------ softmax family
SOFTMAX_ROWS = 37
SOFTMAX_CASES = [(cols, span) for cols in (17, 200, 1500) for span in (100, 200)]  # 16-lane rows, register rows, the long form; logits U(-span, span)


@functools.lru_cache(maxsize=None)
@_quiet
def softmax_case(cols, span):
    """x ~ U(-span, span): exp(x - max) is exactly 0 below -103.98 and subnormal below -87.34 (>= 40 % exact zeros, >= 1 subnormal probability).
    AddSoftmax gets x = xa + addend with a [1, 1, 1, cols] addend row."""
    rng = _rng("softmax", cols, span)
    x = ((rng.random((SOFTMAX_ROWS, cols)) * 2 - 1) * span).astype(F)
    addend = ((rng.random((1, 1, 1, cols)) * 2 - 1) * span * 0.5).astype(F)
    xa = ((rng.random((1, 1, SOFTMAX_ROWS, cols)) * 2 - 1) * span).astype(F)
    # 17 columns over +-200 may hold no subnormal probability by chance (exp(x - max) is cut to 0 below ln(2^-126) = -87.34, so a subnormal comes from
    # exp(-87) = 1.6e-38 divided by a sum >= 2): every fourth row gets a second maximum and its smallest logit at max - 87
    for r in range(0, SOFTMAX_ROWS, 4):
        for row, add in ((x[r], np.zeros(cols, F)), (xa[0, 0, r], addend[0, 0, 0])):
            order = np.argsort(row + add)
            top = (row + add)[order[-1]]
            row[order[1]] = top - add[order[1]]
            row[order[0]] = top - F(87) - add[order[0]]
    return dict(x=x, softmax=ref.softmax(x, lanes=16), log_softmax=norm_rules.log_softmax(x), xa=xa, addend=addend,
                add_softmax=ref.softmax(xa, addend=addend, add_div=SOFTMAX_ROWS, add_mod=1))


def softmax_holds(case):
    a, b = shares(case["softmax"]), shares(case["add_softmax"])
    return all(s["zero"] >= 0.4 and s["sub"] > 0 for s in (a, b)), dict(softmax=a, add_softmax=b)


# ------------------------------------------------------------------------------------------ LayerNorm / InstanceNorm
NORM_BANDS = ("small", "big")   # x in 2^[-72,-66]: (x - mean)^2 is subnormal, the variance vanishes beside epsilon, outputs stay normal;
                                # x in 2^[62,66]: the sum of squares overflows
NORM_RANGE = {"small": (-72, -66), "big": (62, 66)}
LAYER_NORM_ROWS = 29
LAYER_NORM_CASES = [(cols, band) for cols in (100, 768, 2000) for band in NORM_BANDS]
INSTANCE_NORM_CASES = [(inner, band) for inner in (49, 1500) for band in NORM_BANDS]


def _norm_rows(rng, rows, cols, band):
    x = wide(rng, (rows, cols), *NORM_RANGE[band])
    x[1] = x[1, 0]   # constant rows: the variance is exactly 0
    x[rows - 1] = x[rows - 1, 0]
    return x


@functools.lru_cache(maxsize=None)
@_quiet
def layer_norm_case(cols, band):
    rng = _rng("layer_norm", cols, band)
    x, r = _norm_rows(rng, LAYER_NORM_ROWS, cols, band), _norm_rows(rng, LAYER_NORM_ROWS, cols, band)
    g, b = wide(rng, (cols,), -3, 3), wide(rng, (cols,), -3, 3)
    return dict(x=x, r=r, g=g, b=b, plain=ref.layer_norm(x, g, b, 1.0, 0.0, lanes=16), added=ref.layer_norm(ref.add(x, r), g, b, 1.0, 0.0, eps=1e-12, lanes=16))


@functools.lru_cache(maxsize=None)
@_quiet
def instance_norm_case(inner, band):
    rng = _rng("instance_norm", inner, band)
    x = _norm_rows(rng, 6, inner, band).reshape(2, 3, inner)
    scale, bias = wide(rng, (3,), -3, 3), wide(rng, (3,), -3, 3)
    return dict(x=x, scale=scale, bias=bias, want=norm_rules.instance_norm(x, scale, bias, 1e-5))


@_quiet
def norm_holds(band, x, want):
    """On the INPUT, in float32 arithmetic: `small` squares are all subnormal or zero and the outputs normal; `big` sums of squares overflow."""
    x = np.asarray(x, F).reshape(-1, x.shape[-1])
    varied = x[(x != x[:, :1]).any(axis=1)]
    sq = (varied - varied.mean(axis=1, dtype=F, keepdims=True)) ** 2
    if band == "small":
        s = shares(want)
        return bool((sq < TINY).all()) and s["normal"] >= 0.99, s
    return bool(np.isinf(sq.sum(axis=1, dtype=F)).all()), shares(want)


# ------------------------------------------------------------------------------------------ pooling
@functools.lru_cache(maxsize=None)
@_quiet
def pool_case():
    """Input in 2^[-149,-127]: every sum and every quotient is subnormal (>= 90 % nonzero subnormal outputs)."""
    rng = _rng("pool")
    x, xg = wide(rng, (2, 3, 9, 9), -149, -127), wide(rng, (2, 10, 7, 7), -149, -127)
    avg = {cip: ref.average_pool(x, (3, 3), (2, 2), (1, 1, 1, 1), cip, False) for cip in (False, True)}
    return dict(x=x, xg=xg, avg=avg, gap=ref.global_average_pool(xg, lanes=16))


# ------------------------------------------------------------------------------------------ GRU / LSTM
RNN_BANDS = ("rnn_tiny", "saturate")
RNN_CASES = [(lstm, direction, band) for lstm in (False, True) for direction in ("forward", "bidirectional") for band in RNN_BANDS]


def rnn_geometry(lstm, direction):
    return dict(hidden=20, input=32, batch=17, seq=5, direction=direction, bias=False, h0=False, c0=False, mask=7 if lstm else 3)


@functools.lru_cache(maxsize=None)
@_quiet
def rnn_case(lstm, direction, band):
    """rnn_tiny: X in 2^[-149,-135], W and R in 2^[-6,0], no bias: the gates sit at sigmoid(0), the candidate is subnormal, so h is subnormal when it
    goes back into the recurrent product (>= 20 % of Y subnormal).  saturate: X in 2^[4,8], W in 2^[-2,0], R ordinary: the sigmoid is exactly 0 or 1
    through exp's overflow and tanh is +-1 (GRU: >= 50 % of |Y| == 1; LSTM: >= 50 % exact zeros)."""
    c = rnn_geometry(lstm, direction)
    rng = _rng("rnn", lstm, direction, band)
    G, dirs, H = (4 if lstm else 3), (2 if direction == "bidirectional" else 1), c["hidden"]
    if band == "rnn_tiny":
        x, w, r = wide(rng, (c["seq"], c["batch"], c["input"]), -149, -135), wide(rng, (dirs, G * H, c["input"]), -6, 0), wide(rng, (dirs, G * H, H), -6, 0)
    else:
        u = lambda *s, k: ((rng.random(s, dtype=F) - F(0.5)) * F(2 * k)).astype(F)  # noqa: E731
        x, w, r = wide(rng, (c["seq"], c["batch"], c["input"]), 4, 8), wide(rng, (dirs, G * H, c["input"]), -2, 0), u(dirs, G * H, H, k=1 / np.sqrt(H))
    t = dict(x=x, w=w, r=r, b=None, h0=None, c0=None)
    want = rnn_rules.lstm(x, w, r, None, None, None, direction) if lstm else rnn_rules.gru(x, w, r, None, None, direction)
    return dict(t=t, c=c, want=want)


def rnn_holds(lstm, band, case):
    y = case["want"][0]
    s = shares(y)
    if band == "rnn_tiny":
        return s["sub"] >= 0.2, s
    if lstm:
        return s["zero"] >= 0.5, s
    ones = float((np.abs(y) == 1).mean())
    return ones >= 0.5, dict(s, ones=ones)


# ------------------------------------------------------------------------------------------ MatMulNBits
NBITS_CASES = [(rows, k, bs, band) for rows in (1, 4) for (k, bs) in ((256, 32), (144, 16)) for band in ("sub_scales", "big_scales")]
NBITS_COLS = 8


@functools.lru_cache(maxsize=None)
@_quiet
def nbits_case(rows, k, bs, band):
    """sub_scales: every scale below 1e-44 (2^-149 .. 2^-147), lhs in 2^[0,8]: every weight (q - 8) s is subnormal.  big_scales: scales in
    [2^125, 2^126) with codes 4..12 and lhs about 2^-112: 8 s overflows but (q - 8) s, |q - 8| <= 4, does not.  The oracle is finite in both.
    K = 144 leaves a 16-element scalar tail behind one 128-element vector step."""
    rng = _rng("nbits", rows, k, bs, band)
    n = NBITS_COLS
    if band == "sub_scales":
        scales, lhs = wide(rng, (n, k // bs), -149, -148), wide(rng, (rows, k), 0, 8)
        lo, hi = rng.integers(0, 16, (n, k // bs, bs // 2)), rng.integers(0, 16, (n, k // bs, bs // 2))
    else:
        scales, lhs = wide(rng, (n, k // bs), 125, 125), wide(rng, (rows, k), -112, -112)
        lo, hi = rng.integers(4, 13, (n, k // bs, bs // 2)), rng.integers(4, 13, (n, k // bs, bs // 2))
    quant = (lo | (hi << 4)).astype(np.uint8)
    return dict(lhs=lhs, quant=quant, scales=scales, want=ref.matmul_nbits_f32(lhs, quant, scales))


# ------------------------------------------------------------------------------------------ DynamicQuantizeLinear
DQL_INPUTS = ("subnormal", "full_range", "with_inf", "with_nan", "constant", "negative_subnormal")
DQL_STAGED_GEOM = (2, 20, 9, 11, 24, 3, 1, 1)  # N, C, H, W, O, k, pad, stride: the staged form quantises into its consumer's padded image


@_quiet
def dql_input(kind, shape):
    rng = _rng("dql", kind, shape)
    n = int(np.prod(shape))
    if kind == "subnormal":                 # the oracle's scale is subnormal
        x = wide(rng, (n,), -149, -127)
    elif kind == "full_range":              # max - min overflows: the range and the scale are inf
        x = ((rng.random(n) * 2 - 1) * 3e38).astype(F)
        x[:2] = (-3e38, 3e38)
    elif kind == "with_inf":
        x = (rng.random(n, dtype=F) - F(0.5)) * F(6)
        x[n // 3], x[n // 2] = np.inf, -np.inf
    elif kind == "with_nan":                # the min / max drop NaN
        x = (rng.random(n, dtype=F) - F(0.5)) * F(6)
        x[::7] = np.nan
    elif kind == "constant":
        x = np.full(n, 3.0, F)
    else:
        x = -np.abs(wide(rng, (n,), -149, -127))
    return x.astype(F).reshape(shape)


@functools.lru_cache(maxsize=None)
@_quiet
def dql_case(kind, staged):
    x = dql_input(kind, DQL_STAGED_GEOM[:4] if staged else (1000,))
    q, s, z = ref.dynamic_quantize_linear(x)
    return dict(x=x, codes=q, scale=F(s), zero_point=int(z))


# ------------------------------------------------------------------------------------------ ConvIntegerToFloat epilogue
# With a power-of-two scale (float)acc * scale is exact wherever it stays normal, and a fused fma(acc, scale, bias) would give the same bits as the
# multiply and the add rounded one after the other.  The 1.37 cases make the product inexact, so the rounding order shows.
CI2F_SCALES = {"scale_2^-140": 2.0 ** -140, "scale_2^100": 2.0 ** 100, "scale_1.37*2^-140": 1.37 * 2.0 ** -140, "scale_1.37*2^100": 1.37 * 2.0 ** 100}
CI2F_CASES = tuple(CI2F_SCALES)


@functools.lru_cache(maxsize=None)
@_quiet
def ci2f_case(kind):
    """N2 C16 7x7 O8 1x1.  scale about 2^-140 with a subnormal bias: (float)acc * scale is subnormal for |acc| < 2^14 (>= 50 % subnormal outputs);
    scale about 2^100: large, finite.  `biased` = the oracle's cast_scale, then the oracle's Add: two roundings.
    test_range_cases.py shows against exact rational arithmetic that the 1.37 cases tell that from one fused rounding."""
    rng = _rng("ci2f", kind)
    x = rng.integers(0, 256, (2, 16, 7, 7)).astype(np.uint8)
    w = rng.integers(-64, 64, (8, 16, 1, 1)).astype(np.int8)
    small = "-140" in kind
    scale = F(CI2F_SCALES[kind])
    bias = wide(rng, (8,), -149, -130) if small else wide(rng, (8,), 90, 110)
    acc = ref.conv2d_int8(x, w, x_zp=120, pad_mode=ref.PAD_RAW0_I8)
    plain = ref.cast_scale(acc, scale)
    biased = ref.add(plain, np.ascontiguousarray(np.broadcast_to(bias[None, :, None, None], plain.shape)))
    return dict(x=x, w=w, x_zp=np.array(120, np.uint8), scale=np.array(scale, F), bias=bias, acc=acc, plain=plain, biased=biased)
