"""The operand bands of tests/range_cases.py on the CPU oracle (no GPU): every (case, band) pair the device file runs meets its band's condition --
a `tiny` case really produces subnormals, a `huge` one really overflows -- and the oracle itself, never exercised at the ends of the range before,
equals a scalar k-ordered FMA chain evaluated in exact rational arithmetic with one rounding per FMA."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import ref
from tests import range_cases as RC

F = np.float32


# ------------------------------------------------------------------------------------------ exact arithmetic with one float32 rounding
def round_f32(q):
    """A rational (or +-inf / NaN, passed through) rounded once to float32: nearest, ties to even, gradual underflow, overflow to inf."""
    if not isinstance(q, Fraction):
        return q
    if q == 0:
        return Fraction(0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                          # 2^e <= a < 2^(e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)   # below 2^-126 the grid stays at 2^-149
    n = a / quantum
    r = n.numerator // n.denominator
    rem = n - r
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and r & 1):
        r += 1
    v = r * quantum
    if v >= Fraction(2) ** 128:
        return float("inf") if q > 0 else float("-inf")
    return v if q > 0 else -v


def add(x, y):
    """x + y, rounded once; either may be +-inf or NaN."""
    if isinstance(x, Fraction) and isinstance(y, Fraction):
        return round_f32(x + y)
    return float(x) + float(y)          # an infinite or NaN operand: IEEE rules (inf - inf = NaN); a finite partner does not matter


def fma(a, b, acc):
    """a * b + acc with the product exact; a and b finite."""
    if isinstance(acc, Fraction):
        return round_f32(a * b + acc)
    return acc                          # inf + finite = inf, NaN stays


def exact(x):
    return Fraction(float(x))           # float32 -> float64 -> Fraction: both exact


def as_f32(v):
    return F(float(v)) if isinstance(v, Fraction) else F(v)   # v is on the float32 grid, so float() is exact


def same(got, want):
    got, want = np.asarray(got, F), np.asarray(want, F)
    return bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


def chain(products):
    acc = Fraction(0)
    for a, b in products:
        acc = fma(exact(a), exact(b), acc)
    return acc


def test_the_rounding_helper_on_known_values():
    assert round_f32(Fraction(1, 3)) == Fraction(float(F(1) / F(3)))
    assert round_f32(Fraction(2) ** -150) == 0                      # a tie between 0 and 2^-149: to even
    assert round_f32(Fraction(3, 2) * Fraction(2) ** -149) == Fraction(2) ** -148    # tie between 1 and 2 quanta: to even
    assert round_f32(Fraction(2) ** -150 + Fraction(2) ** -200) == Fraction(2) ** -149
    fmax = Fraction(float(np.finfo(F).max))
    assert round_f32(fmax + Fraction(2) ** 102) == fmax             # below the halfway point to 2^128
    assert round_f32(fmax + Fraction(2) ** 103) == float("inf")     # the tie goes to the even neighbour, 2^128: overflow
    assert round_f32(-(Fraction(2) ** 128)) == float("-inf")
    assert np.isnan(add(float("inf"), float("-inf")))
    for v in (1e-40, -3e-39, 1.5, 3e38):
        assert as_f32(round_f32(Fraction(v))) == F(v)


# ------------------------------------------------------------------------------------------ the oracle against the exact chain
def pin_operand(rng, band, role, shape):
    """The band's operand; `huge` with the exponents moved up (both in 2^[59,63]), since a chain of 20 or 9 products of the band proper never overflows."""
    if band == "huge":
        return RC.wide(rng, shape, 59, 63)
    return RC.operand(rng, band, role, shape)


@pytest.mark.parametrize("band", ["tiny", "sub_a", "huge", "spread"])
def test_oracle_gemm_and_conv_equal_the_exact_fma_chain(band):
    """3x20x4 GEMM and a 1-channel 3x3 convolution (padding 1 on a 4x5 image, two output channels: with one the reference takes its depthwise
    sequence of separately rounded multiplies and adds): one depth block, so each output is one k-ordered chain from 0."""
    rng = RC._rng("pin", band)
    a, b = pin_operand(rng, band, "a", (3, 20)), pin_operand(rng, band, "b", (20, 4))
    with np.errstate(all="ignore"):
        got = ref.gemm_f32(a, b)
    want = np.array([[as_f32(chain((a[i, k], b[k, j]) for k in range(20))) for j in range(4)] for i in range(3)], F)
    assert same(got, want), (band, got, want)
    if band in ("tiny", "sub_a"):
        assert (np.abs(want)[want != 0] > 0).any() and RC.shares(want)["zero"] < 0.5, "the micro case degenerated to zeros"
    w, x = pin_operand(rng, band, "a", (2, 1, 3, 3)), pin_operand(rng, band, "b", (1, 1, 4, 5))
    with np.errstate(all="ignore"):
        got = ref.conv2d_f32(x, w, None, pads=(1, 1, 1, 1))
    xp = np.zeros((6, 7), F)
    xp[1:5, 1:6] = x[0, 0]
    want = np.array([[[as_f32(chain((w[o, 0, ky, kx], xp[oy + ky, ox + kx]) for ky in range(3) for kx in range(3))) for ox in range(5)] for oy in range(4)] for o in range(2)], F)
    assert same(got[0], want), (band, got, want)


def test_micro_cases_of_the_pin_reach_subnormals_and_infinities():
    """The chain comparison above is only worth something if the micro cases land where the bands aim."""
    rng = RC._rng("pin", "tiny")
    with np.errstate(all="ignore"):
        y = ref.gemm_f32(pin_operand(rng, "tiny", "a", (3, 20)), pin_operand(rng, "tiny", "b", (20, 4)))
    assert RC.shares(y)["sub"] >= 0.5
    rng = RC._rng("pin", "huge")
    with np.errstate(all="ignore"):
        y = ref.gemm_f32(pin_operand(rng, "huge", "a", (3, 20)), pin_operand(rng, "huge", "b", (20, 4)))
    assert np.isinf(y).any() and np.isfinite(y).any()


@pytest.mark.parametrize("rows", [1, 4])
def test_oracle_matmul_nbits_is_finite_at_scales_whose_eightfold_overflows(rows):
    """Scales in [2^125, 2^126), codes 4..12: 8 s overflows, (q - 8) s does not.  The oracle is finite and equals the chain over the once-rounded weights
    (q - 8) * s: for four rows the blocked GEMM's k-ordered chain (K = 256: one depth block); for one row 64 slots, slot s owning k = s, s + 64, ...,
    folded across 16, 32, 8, 4, 2, 1."""
    c = RC.nbits_case(rows, 256, 32, "big_scales")
    lhs, quant, scales, got = c["lhs"], c["quant"], c["scales"], c["want"]
    assert np.isfinite(got).all() and (np.abs(scales) >= 2.0 ** 125).all() and (np.abs(scales) < 2.0 ** 126).all()
    with np.errstate(over="ignore"):
        assert np.isinf(F(8) * scales).all()
    n = quant.shape[0]
    codes = np.stack([quant & 0xF, quant >> 4], axis=-1).reshape(n, 256).astype(np.int64)   # element 2j in the low nibble
    assert codes.min() >= 4 and codes.max() <= 12
    weight = [[round_f32(Fraction(int(codes[j, k]) - 8) * exact(scales[j, k // 32])) for k in range(256)] for j in range(n)]
    want = np.zeros((rows, n), F)
    for i in range(rows):
        for j in range(n):
            if rows > 1:
                acc = Fraction(0)
                for k in range(256):
                    acc = fma(exact(lhs[i, k]), weight[j][k], acc)
            else:
                slots = [Fraction(0)] * 64
                for k in range(256):
                    slots[k % 64] = fma(exact(lhs[i, k]), weight[j][k], slots[k % 64])
                for d in (16, 32, 8, 4, 2, 1):
                    slots = [add(slots[s], slots[s ^ d]) for s in range(64)]
                acc = slots[0]
            want[i, j] = as_f32(acc)
    assert same(got, want), (got, want)


# ------------------------------------------------------------------------------------------ every (case, band) pair of the device file
def _assert_band(band, cond, what, one_block=False):
    for key, y in cond.items():
        ok, s = RC.band_holds(band, y, one_block)
        assert ok, f"{what} [{key}] does not meet the condition of band {band}: {s}"


@pytest.mark.parametrize("band,shape", RC.GEMM_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gemm_cases_meet_their_band(band, shape):
    c = RC.gemm_case(band, shape)
    _assert_band(band, c["cond"], f"GEMM {shape}")
    if band in ("sub_a", "sub_b"):
        assert RC.all_subnormal(c["a" if band == "sub_a" else "b"])


@pytest.mark.parametrize("name,band", RC.CONV_CASES)
def test_conv_cases_meet_their_band(name, band):
    c = RC.conv_case(name, band)
    _assert_band(band, c["cond"], f"conv {name}", c["one_block"])
    if band in ("sub_a", "sub_b"):
        assert RC.all_subnormal(c["w" if band == "sub_a" else "x"])


@pytest.mark.parametrize("form,band", RC.PAIR_CASES)
def test_pair_cases_meet_their_band(form, band):
    c = RC.pair_case(form, band)
    _assert_band(band, c["cond"], f"pair {form}", c["one_block"])
    if band == "tiny":   # y1 is subnormal where it re-enters the second product
        y1 = c["want1"]
        assert RC.shares(y1)["normal"] <= 0.001 and RC.shares(y1)["sub"] >= 0.4, RC.shares(y1)   # (the rest is what Relu zeroed)
        assert RC.shares(c["want2"])["sub"] >= 0.4, RC.shares(c["want2"])


@pytest.mark.parametrize("name,band", RC.CONVT_CASES)
def test_conv_transpose_cases_meet_their_band(name, band):
    c = RC.convt_case(name, band)
    _assert_band(band, c["cond"], f"ConvTranspose {name}")
    if band == "sub_a":
        assert RC.all_subnormal(c["w"])


@pytest.mark.parametrize("kernel,band", RC.SDPA_CASES)
def test_attention_cases_meet_their_band(kernel, band):
    ok, s = RC.sdpa_holds(band, RC.sdpa_case(kernel, band))
    assert ok, (kernel, band, s)


@pytest.mark.parametrize("cols,span", RC.SOFTMAX_CASES)
def test_softmax_cases_hold_exact_zeros_and_subnormal_probabilities(cols, span):
    ok, s = RC.softmax_holds(RC.softmax_case(cols, span))
    assert ok, (cols, span, s)


@pytest.mark.parametrize("cols,band", RC.LAYER_NORM_CASES)
def test_layer_norm_cases_meet_their_band(cols, band):
    c = RC.layer_norm_case(cols, band)
    for x, want in ((c["x"], c["plain"]), (ref.add(c["x"], c["r"]), c["added"])):
        ok, s = RC.norm_holds(band, x, want)
        assert ok, (cols, band, s)


@pytest.mark.parametrize("inner,band", RC.INSTANCE_NORM_CASES)
def test_instance_norm_cases_meet_their_band(inner, band):
    c = RC.instance_norm_case(inner, band)
    ok, s = RC.norm_holds(band, c["x"], c["want"])
    assert ok, (inner, band, s)


def test_pool_cases_are_subnormal_throughout():
    c = RC.pool_case()
    assert RC.all_subnormal(c["x"]) and RC.all_subnormal(c["xg"])
    for y in (c["avg"][False], c["avg"][True], c["gap"]):
        assert RC.shares(y)["sub"] >= 0.9, RC.shares(y)


@pytest.mark.parametrize("lstm,direction,band", RC.RNN_CASES)
def test_rnn_cases_meet_their_band(lstm, direction, band):
    ok, s = RC.rnn_holds(lstm, band, RC.rnn_case(lstm, direction, band))
    assert ok, (lstm, direction, band, s)


@pytest.mark.parametrize("case", RC.NBITS_CASES, ids=lambda v: "-".join(map(str, v)))
def test_matmul_nbits_cases_are_finite_on_the_oracle(case):
    c = RC.nbits_case(*case)
    assert np.isfinite(c["want"]).all() and (c["want"] != 0).mean() >= 0.9
    if case[3] == "sub_scales":
        assert RC.all_subnormal(c["scales"]) and (np.abs(c["scales"]) < 1e-44).all()
        assert RC.shares(c["want"])["sub"] >= 0.5


@pytest.mark.parametrize("staged", [False, True], ids=["plain", "staged"])
def test_dql_inputs_are_what_they_are_named(staged):
    c = {kind: RC.dql_case(kind, staged) for kind in RC.DQL_INPUTS}
    s = c["subnormal"]["scale"]
    assert 0 < s < RC.TINY                                   # the scale itself is subnormal
    assert np.isinf(c["full_range"]["scale"]) and np.isinf(c["with_inf"]["scale"])
    assert np.isfinite(c["with_nan"]["scale"]) and np.isnan(c["with_nan"]["x"]).any()
    assert len(np.unique(c["with_nan"]["codes"])) > 100     # NaN is dropped by min / max: the other elements still spread over the codes
    assert (c["constant"]["codes"] == 255).all() and c["constant"]["zero_point"] == 0
    assert (c["negative_subnormal"]["x"] < 0).all() and c["negative_subnormal"]["zero_point"] == 255


def test_conv_integer_to_float_cases():
    for kind in ("scale_2^-140", "scale_1.37*2^-140"):
        small = RC.ci2f_case(kind)
        assert RC.shares(small["plain"])["sub"] >= 0.5 and RC.shares(small["biased"])["sub"] >= 0.5 and RC.all_subnormal(small["bias"]), kind
    for kind in ("scale_2^100", "scale_1.37*2^100"):
        large = RC.ci2f_case(kind)
        assert np.isfinite(large["biased"]).all() and (np.abs(large["plain"]) >= 2.0 ** 100).mean() >= 0.9, kind


@pytest.mark.parametrize("kind", RC.CI2F_CASES)
def test_conv_integer_to_float_expectation_rounds_twice(kind):
    """The oracle's cast_scale then Add equal (float)acc * scale rounded, then + bias rounded, in exact rational arithmetic.  With a scale that is no
    power of two, a single rounding of acc * scale + bias gives other bits somewhere: those cases would catch a fused epilogue."""
    c = RC.ci2f_case(kind)
    s = exact(c["scale"])
    two = np.empty(c["acc"].shape, F)
    one = np.empty(c["acc"].shape, F)
    for at in np.ndindex(*c["acc"].shape):
        a, b = Fraction(int(c["acc"][at])), exact(c["bias"][at[1]])
        two[at] = as_f32(add(round_f32(a * s), b))
        one[at] = as_f32(round_f32(a * s + b))
    assert same(c["biased"], two), kind
    if "1.37" in kind:
        assert (one != two).any(), kind
