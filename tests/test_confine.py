"""tests/confine.py on the CPU: `assert_confined` passes on an untouched buffer and names the stray byte in a front guard, a back
guard, a row gap of an `ldc > n` layout, a batch gap and in one of the two 8-bit fills -- the evidence that tests/test_gpu_confine.py
fails on a stray store, without modifying a kernel -- and the ORACLE confines every non-finite input set the GPU tests use: its
non-finite outputs are the stated dependency set and everything else has the bits of the all-finite run.  Where the oracle's own
set differs from the naive one (softmax flushes NaN rows inside `ref.sdpa(flush_nan=True)`; a row holding -Inf stays finite under
Softmax) the oracle's result is the contract and the assertion here says what it is."""
import numpy as np
import pytest

from oracle import ref
from tests import confine as K
from tests import norm_rules as NR

F = np.float32


# ------------------------------------------------------------------------------------------------ the helper
def layout(m=5, n=7, ldc=10, batch=3, c_bs=57, lead=3, front=64, back=96, fill=K.FILL):
    """A host-side stand-in of a Guarded output: (raw, written, region) of a [batch][m][n] float32 tensor with strides (c_bs, ldc, 1)."""
    region = front + 4 * lead
    total = region + 4 * K.span((batch, m, n), (c_bs, ldc, 1)) + back
    raw = np.full(total, fill, np.uint8)
    written = K.strided_mask(total, region, 4, (batch, m, n), (c_bs, ldc, 1))
    raw[written] = 0x3C  # "the kernel wrote its output"
    return raw, written, region


def test_strided_mask_marks_exactly_the_elements():
    raw, written, region = layout()
    assert written.sum() == 3 * 5 * 7 * 4
    assert not written[:region].any() and not written[-96:].any()
    assert written[region] and written[region + 4 * 6 + 3] and not written[region + 4 * 7]  # column 7 of row 0 is the first gap element
    assert written[region + 4 * (57 * 2 + 10 * 4 + 6) + 3] and written.nonzero()[0][-1] == region + 4 * (57 * 2 + 10 * 4 + 6) + 3
    assert K.span((3, 5, 7), (57, 10, 1)) == 57 * 2 + 10 * 4 + 6 + 1
    assert K.strided_mask(64, 0, 4, (0, 3), (3, 1)).sum() == 0
    with pytest.raises(AssertionError, match="does not fit"):
        K.strided_mask(16, 0, 4, (2, 3), (3, 1))
    assert K.dense((2, 3, 4)) == (12, 4, 1)
    assert K.gemm_guard(269) == (128 * 269 + 128) * 4 and K.gemm_guard(8) == K.GUARD_FLAT and K.nchw_guard(143) == 128 * 143 * 4


def test_assert_confined_passes_on_an_untouched_buffer():
    raw, written, region = layout()
    K.assert_confined(raw, written, K.FILL, "untouched", region, 4, (57, 10, 1))
    K.assert_confined(np.full(100, K.FILL, np.uint8), np.zeros(100, bool), K.FILL, "nothing written at all")


@pytest.mark.parametrize("where, byte, text", [
    ("front guard", lambda region: region - 5, r"first at byte -5 relative to the output \(front guard\)"),
    ("lead bytes", lambda region: region - 4 * 3, r"first at byte -12 relative"),
    ("back guard", lambda region: region + 4 * K.span((3, 5, 7), (57, 10, 1)) + 17, r"first at byte \+\d+ relative to the output \(back guard / gap\)"),
    ("row gap", lambda region: region + 4 * (57 * 1 + 10 * 2 + 8) + 1, r"element \(batch 1, row 2, column 8\) of the layout with strides \(57, 10, 1\)"),
    ("batch gap", lambda region: region + 4 * (57 * 1 + 10 * 5 + 3), r"element \(batch 1, row 5, column 3\) of the layout with strides \(57, 10, 1\)"),
])
def test_assert_confined_names_a_stray_byte(where, byte, text):
    raw, written, region = layout()
    at = byte(region)
    assert not written[at], where
    raw[at] = 0x00
    with pytest.raises(AssertionError, match=text) as e:
        K.assert_confined(raw, written, K.FILL, where, region, 4, (57, 10, 1), ("batch", "row", "column"))
    assert "1 bytes outside the output" in str(e.value) and "0x00 instead of the fill 0xff" in str(e.value)


def test_a_stray_saturated_code_cannot_hide_in_both_8_bit_fills():
    """A kernel that stores the saturated code 0xFF one element past a uint8 output: invisible against the fill 0xFF, caught against 0x5A."""
    caught = []
    for fill in K.FILLS_8BIT:
        total, region, n = 256, 64, 37
        raw = np.full(total, fill, np.uint8)
        written = K.strided_mask(total, region, 1, (n,), (1,))
        raw[region:region + n] = 7
        raw[region + n] = 0xFF  # the stray store
        try:
            K.assert_confined(raw, written, fill, f"fill {fill:#x}", region, 1, (1,))
            caught.append(False)
        except AssertionError as e:
            assert f"first at byte +{n} relative" in str(e)
            caught.append(True)
    assert caught == [False, True]


def test_a_gap_is_named_in_the_callers_axis_order():
    """The `[B, S, H, D]` attention output seen as (batch, head, row, column): strides (s * o_rs, d, o_rs, 1) are not descending."""
    s_, h, d, o_rs = 3, 2, 4, 2 * 4 + 1
    strides = (s_ * o_rs, d, o_rs, 1)
    assert K.locate(4 * (1 * s_ * o_rs + 2 * o_rs + 1 * d + 3), 4, strides) == (1, 1, 2, 3)
    total = 4 * K.span((2, h, s_, d), strides) + 32
    raw, written = np.full(total, K.FILL, np.uint8), K.strided_mask(total, 0, 4, (2, h, s_, d), strides)
    raw[4 * (s_ * o_rs + o_rs + 2 * d)] = 0  # the padding element behind row 1 of batch 1
    with pytest.raises(AssertionError, match=r"element \(batch 1, head 2, row 1, column 0\)"):
        K.assert_confined(raw, written, K.FILL, "sdpa", 0, 4, strides, ("batch", "head", "row", "column"))


def test_bits_equal_has_no_tolerance():
    a = np.array([1.0, 0.0, np.nan, np.inf], F)
    K.bits_equal(a, np.array([1.0, -0.0, np.nan, np.inf], F), "same")
    for other in ([np.nextafter(F(1), F(2)), 0, np.nan, np.inf], [1, 0, 0, np.inf], [1, 0, np.nan, -np.inf]):
        with pytest.raises(AssertionError, match="1 of 4 elements differ"):
            K.bits_equal(a, np.array(other, F), "different")
    with pytest.raises(AssertionError):
        K.bits_equal(np.zeros(3, np.int32), np.zeros(3, np.float32), "dtype")


# ------------------------------------------------------------------------------------------------ the oracle confines what the GPU tests feed it
def confined(poisoned, clean, dep, what, exact=True):
    """`poisoned`'s non-finite set is `dep` (exact) or inside it, and outside `dep` it has the bits of `clean`."""
    bad = ~np.isfinite(poisoned)
    assert np.isfinite(clean).all(), what
    if exact:
        assert np.array_equal(bad, dep), (what, int(bad.sum()), int(dep.sum()))
    else:
        assert not (bad & ~dep).any(), what
    assert np.array_equal(poisoned[~dep].view(np.int32), clean[~dep].view(np.int32)), what


@pytest.mark.parametrize("m, k, n", K.GEMM_NONFINITE_SHAPES + [(33, 17, 31), (70, 300, 130)])
def test_oracle_gemm_confines_nan_rows_and_columns(m, k, n):
    a, b = K.seeded((m, k), 5), K.seeded((k, n), 6)
    clean = ref.gemm_f32(a, b)
    an, bn, dep = K.gemm_nonfinite(a, b)
    confined(ref.gemm_f32(an, bn), clean, dep, "plain")
    bias = K.seeded((n,), 7)
    confined(ref.gemm_f32(an, bn, bias=bias, bias_kind=ref.BIAS_PER_COL), ref.gemm_f32(a, b, bias=bias, bias_kind=ref.BIAS_PER_COL), dep, "bias")
    # batched: a NaN slice of A reaches its own product only (the products are independent calls of the oracle)
    confined(ref.gemm_f32(np.full_like(a, np.nan), b), clean, np.ones((m, n), bool), "NaN slice")


@pytest.mark.parametrize("name", list(K.CONV_NONFINITE_CASES))
def test_oracle_conv_confines_a_nan_image_and_inf_pixels(name):
    case = K.CONV_NONFINITE_CASES[name]
    n, c, h, w, o, kh, kw, pads, strides, dil, groups = case
    x, wt, b = K.conv_operands(case)
    assert (wt != 0).all()
    clean = ref.conv2d_f32(x, wt, b, pads=pads, strides=strides, dilations=dil, groups=groups)
    xn, mask = K.conv_nonfinite(x)
    dep = K.conv_dependency(mask, wt.shape, pads, strides, dil, groups)
    assert dep.shape == clean.shape and dep[1].all() and dep[0].any() and not dep[0].all()
    if n > 2:
        assert dep[-1].any() and not dep[-1].all()
    confined(ref.conv2d_f32(xn, wt, b, pads=pads, strides=strides, dilations=dil, groups=groups), clean, dep, name)


def test_oracle_conv_transpose_confines_a_nan_image():
    x, wt = K.seeded((2, 4, 5, 7), 1), K.seeded((4, 3, 4, 4), 2)
    clean = ref.conv_transpose2d_f32(x, wt, None, (1, 1, 1, 1), (2, 2))
    xn = x.copy()
    xn[1] = np.nan
    dep = np.zeros(clean.shape, bool)
    dep[1] = True
    confined(ref.conv_transpose2d_f32(xn, wt, None, (1, 1, 1, 1), (2, 2)), clean, dep, "conv transpose")


@pytest.mark.parametrize("s, t, d", [(5, 7, 32), (33, 129, 64), (1, 1, 32), (16, 128, 64)])
def test_oracle_sdpa_confines_a_nan_key_to_its_head(s, t, d):
    """flush_nan = True (sdpa_head) turns the NaN probabilities into zeros: out[1, 0] is then FINITE (all zero) -- the oracle's set, not the
    naive one, is the contract; without the flush it is all NaN.  Either way nothing outside out[1, 0] moves."""
    q, k, v = K.sdpa_operands(2, 2, s, t, d)
    kn = K.sdpa_nonfinite(k)
    dep = np.zeros((2, 2, s, d), bool)
    dep[1, 0] = True
    for mask in (None, K.sdpa_trailing_mask(2, t, t // 2)):
        for flush in (True, False):
            clean = ref.sdpa(q, k, v, mask=mask, flush_nan=flush)
            got = ref.sdpa(q, kn, v, mask=mask, flush_nan=flush)
            confined(got, clean, dep, f"sdpa flush {flush}", exact=not flush)
            assert (got[1, 0] == 0).all() if flush else np.isnan(got[1, 0]).all()


@pytest.mark.parametrize("cols", K.ROWS_NONFINITE_COLS)
def test_oracle_row_wise_operators_keep_non_finite_rows_to_themselves(cols):
    """Row 1 all NaN -> a NaN row; a +Inf element makes its row NaN under Softmax / LayerNormalization; a -Inf element among finite
    values leaves a FINITE Softmax row (probability 0) and a NaN LayerNormalization row.  Rows 0 and 4 keep their bits."""
    x = K.seeded((5, cols), 3, 4.0)
    xn, rows = K.rows_nonfinite(x)
    dep = np.broadcast_to(rows[:, None], x.shape)
    g, b = K.seeded((cols,), 4), K.seeded((cols,), 5)
    for what, fn in (("softmax", lambda v: ref.softmax(v)), ("layer_norm", lambda v: ref.layer_norm(v, g, b)),
                     ("add_layer_norm", lambda v: ref.layer_norm(ref.add(v, x), g, b)), ("log_softmax", lambda v: NR.log_softmax(v))):
        with np.errstate(all="ignore"):
            got, clean = fn(xn), fn(x)
        confined(got, clean, dep, what, exact=False)
        assert np.isnan(got[1]).all() and not np.isfinite(got[2]).all(), what
    assert np.isfinite(ref.softmax(xn)[3]).all() and ref.softmax(xn)[3, -1] == 0
    assert np.isnan(ref.layer_norm(xn, g, b)[3]).all()


@pytest.mark.parametrize("value", [np.nan, -np.inf, np.inf])
def test_oracle_pooling_confines_a_corner_pixel(value):
    x = K.seeded((2, 3, 12, 12), 8)
    xn = K.pool_nonfinite(x, value)
    dep = np.zeros((2, 3, 6, 6), bool)
    dep[0, 0, 0, 0] = True
    for what, fn in (("max", lambda v: ref.max_pool(v, (3, 3), (2, 2), (1, 1, 1, 1))), ("average", lambda v: ref.average_pool(v, (3, 3), (2, 2), (1, 1, 1, 1)))):
        got = fn(xn)
        confined(got, fn(x), dep, what, exact=False)
        if what == "average" or value == np.inf:
            assert not np.isfinite(got[0, 0, 0, 0])
    assert np.isfinite(ref.max_pool(K.pool_nonfinite(x, -np.inf), (3, 3), (2, 2), (1, 1, 1, 1))).all()  # -Inf loses every comparison


@pytest.mark.parametrize("lstm", [False, True], ids=["gru", "lstm"])
@pytest.mark.parametrize("hidden", [3, 20])
def test_restated_rnn_keeps_a_nan_batch_row_to_itself(lstm, hidden):
    """Batch row 3 of x NaN at t = 0 (tests/rnn_rules.py is the expectation of the recurrent layers): only batch row 3 of Y, Y_h (and Y_c) is affected --
    the reverse direction meets t = 0 last, so there Y[t > 0] of row 3 stays finite too."""
    from tests import rnn_rules as R
    rng = np.random.default_rng(hidden)
    seq, batch, n_in, G = 3, 17, 6, 4 if lstm else 3
    u = lambda *s: ((rng.random(s, dtype=F) - F(0.5)) * F(0.8)).astype(F)
    x, w, r, b = u(seq, batch, n_in), u(2, G * hidden, n_in), u(2, G * hidden, hidden), u(2, 2 * G * hidden)
    run = (lambda v: R.lstm(v, w, r, b, direction="bidirectional")) if lstm else (lambda v: R.gru(v, w, r, b, direction="bidirectional"))
    clean = run(x)
    xn = x.copy()
    xn[0, 3] = np.nan
    with np.errstate(all="ignore"):
        got = run(xn)
    for g, c in zip(got, clean):
        dep = np.zeros(g.shape, bool)
        dep[..., 3, :] = True
        confined(g, c, dep, "rnn", exact=False)
    assert np.isnan(got[0][:, 0, 3]).all() and np.isnan(got[0][0, 1, 3]).all() and np.isfinite(got[0][1:, 1, 3]).all()
    assert np.isnan(got[1][:, 3]).all()
