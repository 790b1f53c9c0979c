"""The f32 kernels on operands at the ends of the range (tests/range_cases.py): subnormal inputs, intermediates and outputs, overflowing sums, inf - inf,
and exponents 80 binades apart -- bit for bit against the CPU oracle, which keeps subnormals.  tests/test_range_cases.py asserts on the CPU that every
case here lands where its band aims.

Comparison rule: the project's bits_equal (equal values, NaNs coincide; payloads and the sign of zero are not part of the contract).  A failure names the
family, band, variant or path, and the first differing element with both values in hex.

Every family proves that it ran the kernel it names: the launches are profiled and the kernel name asserted.  A forced GEMM variant silently runs as
variant 3 on a shape outside its form, so the variant sweeps state, next to each variant or split mode, the kernel that must have run."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref
from rten_amd import lib as L
from rten_amd import ops
from rten_amd.tensor import DeviceTensor
from tests import range_cases as RC
from tests.test_gpu_norm import PATHS as INSTANCE_NORM_PATHS, run_instance_norm
from tests.test_gpu_parity import bits_equal, dev, gpu_conv, gpu_gemm
from tests.test_gpu_rnn import run_abi
from tests.test_gpu_round3 import staged_image

pytestmark = pytest.mark.gpu


def same_bits(got, want, what):
    try:
        bits_equal(got, want)
    except AssertionError as e:
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        if got.shape != want.shape:
            raise AssertionError(f"{what}: {e}") from None
        bad = got != want
        if got.dtype == np.float32:
            bad &= ~(np.isnan(got) & np.isnan(want))
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        view = {4: np.uint32, 1: np.uint8}[got.dtype.itemsize]
        raise AssertionError(f"{what}: {e}; first differing element {at}: got {int(got.view(view)[at]):#010x} ({got[at]!r}), "
                             f"expected {int(want.view(view)[at]):#010x} ({want[at]!r})") from None


class launched:
    """with launched(ctx) as k: ...   ->  k.names = the kernels launched inside."""

    def __init__(self, ctx):
        self.ctx, self.names = ctx, set()

    def __enter__(self):
        self.ctx.profile_reset()
        self.ctx.profile(True)
        return self

    def __exit__(self, *exc):
        self.ctx.sync()
        self.ctx.profile(False)
        self.names = {r["kernel"] for r in self.ctx.profile_report()}
        self.ctx.profile_reset()
        return False

    def ran(self, prefix):
        return any(n.startswith(prefix) for n in self.names)


# One kernel-name prefix per f32 GEMM translation unit.
REG, DMA, DMA16, WS, WAVE, PERS = "igemm_f32_kernel<", "igemm_f32_dma_kernel<", "igemm_f32_dma16_kernel<", "igemm_f32_ws_kernel<", "igemm_f32_wave_kernel<", "igemm_f32_pers_kernel<"
THIN, PATCH, SMALLM, STEM, LEAN = "igemm_f32_thin_kernel<", "igemm_f32_patch_kernel<", "gemm_f32_smallm_kernel<", "conv_small_c_f32_kernel<", "igemm_f32_lean_kernel<"


def split_k_producers(names, prefix):
    """Kernels of one family launched as split-K producers: the launch mode is the template's fifth argument, 2 = producer."""
    return [n for n in names if n.startswith(prefix) and n[len(prefix):].rstrip(">").split(",")[4] == "2"]


GEMM_UNITS = (REG, DMA, DMA16, WS, WAVE, PERS, THIN, PATCH, SMALLM, STEM, LEAN)

# The kernel each variant runs on the `patch` convolution with prepacked weights (k-major A, im2col B with tap masks, K = 360 > 256):
CONV_VARIANT_KERNEL = {
    **{v: DMA for v in range(0, 4)},      # three-stage LDS-DMA
    **{v: REG for v in range(4, 8)},      # register-staged
    **{v: WS for v in range(8, 12)},      # wave-specialised
    **{v: DMA for v in range(12, 20)},    # four stages; fragments-first issue
    **{v: DMA16 for v in range(20, 24)},  # 16x16x4 MFMAs
    24: WAVE, 25: WAVE, 26: WAVE,         # one wave per 64x64 tile
    27: DMA,                              # two stages
    28: DMA, 29: DMA,                     # 32x32 wave tiles take a dense B only: an im2col B runs as variant 3
    30: PATCH,                            # image patches
    31: DMA, 32: DMA,                     # small-M and stem forms belong to other entry shapes: variant 3 here
}


def n_variants(ctx):
    return ctx.lib.rten_hip_num_gemm_variants()


# ------------------------------------------------------------------------------------------ GEMM
def _layouts(a, b):
    at, bt = np.ascontiguousarray(a.T).T, np.ascontiguousarray(b.T).T
    return (("a b", a, b), ("aT b", at, b), ("a bT", a, bt), ("aT bT", at, bt))


def _epilogue(ctx, c, b, variant=None):
    return {act: gpu_gemm(ctx, c["a"], b, c=c["c"], alpha=0.5, beta=2.0, bias=c["bias"], bias_kind=L.BIAS_PER_COL, act=code, variant=variant)
            for act, code in (("relu", L.ACT_RELU), ("gelu", L.ACT_GELU))}


@pytest.mark.parametrize("band", RC.MATRIX_BANDS)
def test_gemm_every_variant_split_plan_layout_and_epilogue(ctx, band):
    """(70, 300, 130): N is no multiple of 4, so every operand layout takes the scalar loaders and with them the register-staged kernel, whatever the variant
    (its tile shape still changes); split plans add that kernel's split-K producers and the ordered fixup."""
    c = RC.gemm_case(band, RC.GEMM_SHAPE)
    a, b, want = c["a"], c["b"], c["plain"]
    with launched(ctx) as k:
        for v in range(n_variants(ctx)):
            same_bits(gpu_gemm(ctx, a, b, variant=v), want, f"GEMM {band} variant {v}")  # (31, the small-M form, stops at M = 64: variant 3 here)
    assert k.ran(REG) and not any(k.ran(p) for p in GEMM_UNITS if p != REG), k.names
    try:
        for mode, groups in ((1, 2), (2, 2), (2, 3), (5, 2), (6, 2)):
            ctx.call("rten_hip_set_gemm_split", mode, groups)
            with launched(ctx) as k:
                for v in (0, 3, 24):
                    same_bits(gpu_gemm(ctx, a, b, variant=v), want, f"GEMM {band} split plan ({mode}, {groups}) variant {v}")
            assert k.ran(REG), k.names
            # six tiles at most, fewer than one round of the chip: plan 1 (split the tiles past the last whole round) and plan 2 (split every tile) both cut every tile
            # at the depth-block boundary (K = 300: two blocks); the persistent modes are convolution plans and run the whole-tile kernel here
            assert bool(split_k_producers(k.names, REG)) == (mode in (1, 2)), (mode, k.names)
    finally:
        ctx.call("rten_hip_set_gemm_split", 3, 1)
    for name, aa, bb in _layouts(a, b):
        same_bits(gpu_gemm(ctx, aa, bb), want, f"GEMM {band} layout {name}")
    for act, got in _epilogue(ctx, c, b).items():
        same_bits(got, c[act], f"GEMM {band} alpha/beta/C/column bias + {act}")


# The kernel each variant runs on a dense GEMM whose operands the 16-byte loaders take (A stored m-major, M and N multiples of 4, K = 300 > 256):
DENSE_VARIANT_KERNEL = {
    **{v: DMA for v in range(0, 4)},      # three-stage LDS-DMA
    **{v: REG for v in range(4, 8)},      # register-staged
    **{v: WS for v in range(8, 12)},      # wave-specialised
    **{v: DMA for v in range(12, 20)},    # four stages; fragments-first issue
    **{v: DMA16 for v in range(20, 24)},  # 16x16x4 MFMAs
    24: WAVE, 25: WAVE, 26: WAVE,         # one wave per 64x64 tile
    27: DMA,                              # two stages
    28: WAVE, 29: WAVE,                   # one wave per 32x32 tile: the dense B they are built for (wave flavours 4 and 5, the name's last argument)
    30: DMA,                              # image patches need an im2col B: variant 3 here
    31: DMA, 32: DMA,                     # M = 72 is past the small-M form, and the stem form is a convolution's: variant 3 here
}


@pytest.mark.parametrize("band", RC.MATRIX_BANDS)
def test_gemm_dense_operands_every_variant_runs_its_own_kernel(ctx, band):
    """(72, 300, 132) with A stored m-major: the 16-byte loaders, so each variant runs the kernel DENSE_VARIANT_KERNEL states on a dense (not im2col) B --
    the 32x32 wave tiles of variants 28 and 29 among them, which no convolution reaches.  Six 64x64 tiles are far fewer than the chip's units, so the
    automatic plan cuts the tiles at the depth-block boundary wherever the kernel family has a split-K form."""
    c = RC.gemm_case(band, RC.DENSE_SHAPE)
    at, b, want = np.ascontiguousarray(c["a"].T).T, c["b"], c["plain"]
    for v in range(n_variants(ctx)):
        with launched(ctx) as k:
            same_bits(gpu_gemm(ctx, at, b, variant=v), want, f"dense GEMM {band} variant {v}")
        expect = DENSE_VARIANT_KERNEL[v]
        assert k.ran(expect) and not any(k.ran(p) for p in GEMM_UNITS if p != expect), (v, k.names)
        if v in (28, 29):
            assert {n.rstrip(">").split(",")[-1] for n in k.names if n.startswith(WAVE)} == {str(v - 24)}, (v, k.names)
    for v in (3, 8, 20, 24, 28):  # one variant per kernel family: the fused epilogue
        for act, code in (("relu", L.ACT_RELU), ("gelu", L.ACT_GELU)):
            got = gpu_gemm(ctx, at, b, c=c["c"], alpha=0.5, beta=2.0, bias=c["bias"], bias_kind=L.BIAS_PER_COL, act=code, variant=v)
            same_bits(got, c[act], f"dense GEMM {band} variant {v} alpha/beta/C/column bias + {act}")
    with launched(ctx) as k:  # A row-major (k-contiguous, K a multiple of 4) is the 16-byte loaders' other A layout
        same_bits(gpu_gemm(ctx, c["a"], b, variant=3), want, f"dense GEMM {band} row-major A variant 3")
    assert k.ran(DMA) and not k.ran(REG), k.names
    try:
        ctx.call("rten_hip_set_gemm_split", 5, 2)
        with launched(ctx) as k:
            for v in (3, 20):  # the persistent walk of the tile list, three-stage and 16x16x4 forms
                same_bits(gpu_gemm(ctx, at, b, variant=v), want, f"dense GEMM {band} split plan (5, 2) variant {v}")
        assert k.ran(PERS) and not k.ran(DMA) and not k.ran(DMA16), k.names
    finally:
        ctx.call("rten_hip_set_gemm_split", 3, 1)


@pytest.mark.parametrize("band", RC.MATRIX_BANDS)
def test_gemm_small_m_parks_and_folds_three_depth_blocks(ctx, band):
    c = RC.gemm_case(band, RC.SMALLM_SHAPE)
    with launched(ctx) as k:
        for name, aa, bb in _layouts(c["a"], c["b"]):
            same_bits(gpu_gemm(ctx, aa, bb, variant=31), c["plain"], f"small-M GEMM {band} layout {name}")
        for act, got in _epilogue(ctx, c, c["bt"], variant=31).items():
            same_bits(got, c[act], f"small-M GEMM {band} alpha/beta/C/column bias + {act}")
    assert k.names and all(n.startswith(SMALLM) for n in k.names), k.names
    same_bits(gpu_gemm(ctx, c["a"], c["b"], variant=3), c["plain"], f"GEMM {band} (16, 600, 40) variant 3")  # the blocked kernels on the same three blocks


@pytest.mark.parametrize("band", RC.MATRIX_BANDS)
def test_gemm_one_row_order(ctx, band):
    c = RC.gemm_case(band, RC.ONE_ROW_SHAPE)
    for tag, bb, kernel in (("", c["b"], "gemv_cols_kernel"), ("_bt", c["bt"], "gemv_transposed_kernel")):
        with launched(ctx) as k:
            same_bits(gpu_gemm(ctx, c["a"], bb), c["plain" + tag], f"one-row GEMM {band} {kernel}")
            for act, got in _epilogue(ctx, c, bb).items():
                same_bits(got, c[act + tag], f"one-row GEMM {band} {kernel} alpha/beta/C/bias + {act}")
        assert k.names == {kernel}, k.names


# ------------------------------------------------------------------------------------------ convolution
def _conv(ctx, c, form, **kw):
    if form == "plain":
        return gpu_conv(ctx, c["x"], c["w"], None, c["pads"], c["strides"], (1, 1), c["groups"], **kw)
    return gpu_conv(ctx, c["x"], c["w"], c["bias"], c["pads"], c["strides"], (1, 1), c["groups"], residual=c["res"], relu=True, **kw)


@pytest.mark.parametrize("band", RC.MATRIX_BANDS)
def test_conv_every_variant_prepacked_and_not(ctx, band):
    """N1 C40 9x9 O70 3x3 p1 (K = 360: two depth blocks; 81 columns: ragged tiles).  Prepacked weights: each variant runs the kernel CONV_VARIANT_KERNEL
    states.  Plain weights are loaded by the scalar loaders: the register-staged kernel for every variant."""
    c = RC.conv_case("patch", band)
    for v in range(n_variants(ctx)):
        with launched(ctx) as k:
            for form in ("plain", "full"):
                same_bits(_conv(ctx, c, form, variant=v), c[form], f"conv {band} variant {v} prepacked, {form}")
        expect = CONV_VARIANT_KERNEL[v]
        assert k.ran(expect) and not any(k.ran(p) for p in GEMM_UNITS if p != expect), (v, k.names)
    with launched(ctx) as k:
        for v in range(n_variants(ctx)):
            for form in ("plain", "full"):
                same_bits(_conv(ctx, c, form, variant=v, prepack=False), c[form], f"conv {band} variant {v} plain weights, {form}")
    assert k.ran(REG) and not any(k.ran(p) for p in GEMM_UNITS if p != REG), k.names


def _plans(ctx, c, band, what, plans):
    try:
        for (mode, groups), variant, expect in plans:
            ctx.call("rten_hip_set_gemm_split", mode, groups)
            with launched(ctx) as k:
                for form in ("plain", "full"):
                    same_bits(_conv(ctx, c, form, variant=variant), c[form], f"conv {what} {band} split plan ({mode}, {groups}) variant {variant}, {form}")
            assert split_k_producers(k.names, DMA) if expect == "split-K producers" else k.ran(expect), (mode, groups, variant, k.names)
    finally:
        ctx.call("rten_hip_set_gemm_split", 3, 1)


@pytest.mark.parametrize("band", RC.MATRIX_BANDS)
def test_conv_whole_rounds_and_thin_tail(ctx, band):
    """N1 C8 92x92 O70 3x3 p1: 266 tiles of 64x64.  Split mode 4 sends the columns past the whole round to the thin 16x64 kernel; mode 5 walks the tile list
    persistently (three-stage and 16x16x4 forms)."""
    _plans(ctx, RC.conv_case("rounds", band), band, "92x92", (((4, 1), 3, THIN), ((5, 2), 3, PERS), ((5, 2), 20, PERS)))


@pytest.mark.parametrize("band", RC.MATRIX_BANDS)
def test_conv_lean_persistent_and_split_k_plans(ctx, band):
    """N1 C32 9x9 O70 3x3 p1 (K = 288: two depth blocks of whole 32-deep k-tiles; four tiles).  Mode 6 is the lean persistent kernel, mode 5 the persistent
    one across a depth-block fold, (2, 2) and (1, 2) split every tile in two K groups folded by the last arrival."""
    _plans(ctx, RC.conv_case("lean", band), band, "C32 9x9", (((6, 2), 3, LEAN), ((5, 2), 3, PERS), ((2, 2), 3, "split-K producers"), ((1, 2), 3, "split-K producers"),
                                                              ((2, 2), 24, WAVE), ((2, 2), 30, PATCH)))


@pytest.mark.parametrize("band", RC.MATRIX_BANDS)
def test_conv_stem(ctx, band):
    c = RC.conv_case("stem", band)
    for v, expect in ((32, STEM), (-1, STEM), (3, DMA)):
        with launched(ctx) as k:
            same_bits(_conv(ctx, c, "plain", variant=v), c["plain"], f"stem conv {band} variant {v}")
            same_bits(gpu_conv(ctx, c["x"], c["w"], c["bias"], c["pads"], c["strides"], relu=True, variant=v), ref.conv2d_f32(c["x"], c["w"], c["bias"], pads=c["pads"], strides=c["strides"], relu=True),
                      f"stem conv {band} variant {v} bias + Relu")
        assert k.ran(expect) and (expect == STEM) != k.ran(DMA), (v, k.names)


@pytest.mark.parametrize("name,band", [(n, b) for n, b in RC.CONV_CASES if n.startswith("dw_")])
def test_depthwise(ctx, name, band):
    """dw_9x8 and dw_6x8 take the streaming kernel (rows of whole 16-byte groups), dw_9x7 the four-rows-per-thread one; both are profiled under one name."""
    c = RC.conv_case(name, band)
    with launched(ctx) as k:
        for prepack in (True, False):
            for form in ("plain", "full"):
                same_bits(_conv(ctx, c, form, prepack=prepack), c[form], f"depthwise {name} {band} prepack={prepack} {form}")
    assert "depthwise_conv2d_f32" in k.names and not any(k.ran(p) for p in GEMM_UNITS), k.names


# ------------------------------------------------------------------------------------------ pair kernels
def _desc(n, c, h, w, o):
    return L.Conv2dDesc(n, c, h, w, o, 1, 1, (C.c_int32 * 4)(0, 0, 0, 0), 1, 1, 1, 1, 1, h, w)


def _packed(ctx, d, w):
    wd = dev(ctx, w)
    p = DeviceTensor(ctx, (ctx.lib.rten_hip_conv2d_f32_packed_bytes(C.byref(d)) // 4,), np.float32)
    ctx.call("rten_hip_conv2d_f32_prepack", C.byref(d), wd.vp, p.vp)
    ctx.sync()
    return p


@pytest.mark.parametrize("form,band", RC.PAIR_CASES)
def test_pair_kernels_both_outputs(ctx, form, band):
    """y1 goes to LDS and comes back as the second product's MFMA operand: in `tiny` it is subnormal there (asserted on the oracle's y1 in test_range_cases)."""
    c = RC.pair_case(form, band)
    N, C1, H, W, M1, _ = RC.PAIR_GEOM
    M2 = c["w2"].shape[0]
    d1, d2 = _desc(N, C1, H, W, M1), _desc(N, M1, H, W, M2)
    xd, p1, p2, b1, b2 = dev(ctx, c["x"]), _packed(ctx, d1, c["w1"]), _packed(ctx, d2, c["w2"]), dev(ctx, c["b1"]), dev(ctx, c["b2"])
    y1, y2 = DeviceTensor(ctx, (N, M1, H, W), np.float32), DeviceTensor(ctx, (N, M2, H, W), np.float32)
    with launched(ctx) as k:
        if form == "pair":
            assert ctx.lib.rten_hip_conv2d_f32_pair_supported(C.byref(d1), C.byref(d2)) == 1
            rd = dev(ctx, c["r"])
            ctx.call("rten_hip_conv2d_f32_pair", C.byref(d1), xd.vp, p1.vp, b1.vp, rd.vp, L.CONV_RELU | L.CONV_RESIDUAL, y1.vp, C.byref(d2), p2.vp, b2.vp, L.CONV_RELU, y2.vp)
        else:
            ds = _desc(N, C1, H, W, M1)
            assert ctx.lib.rten_hip_conv2d_f32_pair_shortcut_supported(C.byref(d1), C.byref(ds), C.byref(d2)) == 1
            xs, ps, bs = dev(ctx, c["xs"]), _packed(ctx, ds, c["ws"]), dev(ctx, c["bs"])
            ctx.call("rten_hip_conv2d_f32_pair_shortcut", C.byref(d1), xd.vp, p1.vp, b1.vp, C.byref(ds), xs.vp, ps.vp, bs.vp, L.CONV_RELU, y1.vp, C.byref(d2), p2.vp, b2.vp, L.CONV_RELU, y2.vp)
    assert ("conv_pair_f32_kernel" if form == "pair" else "conv_pair_f32_kernel<shortcut>") in k.names, k.names
    same_bits(y1.numpy(), c["want1"], f"{form} kernel {band} first output")
    same_bits(y2.numpy(), c["want2"], f"{form} kernel {band} second output")


# ------------------------------------------------------------------------------------------ ConvTranspose
@pytest.mark.parametrize("name,band", RC.CONVT_CASES)
def test_conv_transpose(ctx, name, band):
    c = RC.convt_case(name, band)
    pads, strides, dil, groups, opad = c["geom"]
    op = ops.ConvTranspose(padding=list(pads), groups=groups, strides=list(strides), dilations=list(dil), output_padding=list(opad))
    with launched(ctx) as k:
        same_bits(op.run(ctx, [dev(ctx, c["x"]), dev(ctx, c["w"])])[0].numpy(), c["plain"], f"ConvTranspose {name} {band}")
        same_bits(op.run(ctx, [dev(ctx, c["x"]), dev(ctx, c["w"]), dev(ctx, c["bias"])])[0].numpy(), c["biased"], f"ConvTranspose {name} {band} with bias")
    assert ("conv_transpose_fused_kernel" in k.names) == (name == "fused") and ("col2im_f32" in k.names) == (name == "col2im"), k.names


# ------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("kernel,band", RC.SDPA_CASES)
def test_attention_one_kernel_and_composed_paths(ctx, kernel, band):
    c = RC.sdpa_case(kernel, band)
    B, H, S, T, hd = RC.SDPA_SHAPES[kernel]
    qd, kd, vd, md = dev(ctx, c["q"]), dev(ctx, c["k"]), dev(ctx, c["v"]), dev(ctx, c["mask"])
    for path in (2, 1):  # 2 = the one-kernel form wherever it covers the shape; 1 = composed GEMM / softmax / GEMM
        for masked in (False, True):
            for flush in (False, True):
                d = L.SdpaDesc(B, H, S, T, hd, hd, H * S * hd, S * hd, hd, H * T * hd, T * hd, hd, H * T * hd, T * hd, hd, H * S * hd, S * hd, hd,
                               T if masked else 0, 0, c["scale"], 1 if flush else 0)
                out = DeviceTensor(ctx, (B, H, S, hd), np.float32)
                ctx.call("rten_hip_set_sdpa_path", path)
                try:
                    with launched(ctx) as k:
                        ctx.call("rten_hip_sdpa_f32", C.byref(d), qd.vp, kd.vp, vd.vp, md.vp if masked else None, out.vp)
                finally:
                    ctx.call("rten_hip_set_sdpa_path", 0)
                fused = {n for n in k.names if n.startswith("sdpa_fused")}
                assert fused == ({kernel} if path == 2 else set()), (path, k.names)
                same_bits(out.numpy(), c["want"][(masked, flush)], f"attention {kernel if path == 2 else 'composed path on the shape of ' + kernel} {band} mask={masked} flush={flush}")


# ------------------------------------------------------------------------------------------ softmax family
@pytest.mark.parametrize("cols,span", RC.SOFTMAX_CASES)
def test_softmax_log_softmax_add_softmax(ctx, cols, span):
    c = RC.softmax_case(cols, span)
    what = f"{RC.SOFTMAX_ROWS} x {cols} logits in +-{span}"
    with launched(ctx) as k:
        same_bits(ops.Softmax(axis=-1).run(ctx, [dev(ctx, c["x"])])[0].numpy(), c["softmax"], f"Softmax {what}")
        same_bits(ops.AddSoftmax().run(ctx, [dev(ctx, c["xa"]), dev(ctx, c["addend"])])[0].numpy(), c["add_softmax"], f"AddSoftmax {what}")
    assert "softmax_f32" in k.names and "log_softmax_f32" not in k.names, k.names
    with launched(ctx) as k:
        same_bits(ops.LogSoftmax().run(ctx, [dev(ctx, c["x"])])[0].numpy(), c["log_softmax"], f"LogSoftmax {what}")
    assert k.names == {"log_softmax_f32"}, k.names


# ------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("cols,band", RC.LAYER_NORM_CASES)
def test_layer_norm_and_add_layer_norm(ctx, cols, band):
    c = RC.layer_norm_case(cols, band)
    rows = RC.LAYER_NORM_ROWS
    with launched(ctx) as k:
        got = ops.LayerNormalization(axis=-1).run(ctx, [dev(ctx, c["x"]), dev(ctx, c["g"]), dev(ctx, c["b"])])[0].numpy()
    assert k.names == {"layer_norm_f32"}, k.names
    same_bits(got, c["plain"], f"LayerNorm {cols} columns, x {band}")
    xd, rd, gd, bd = dev(ctx, c["x"]), dev(ctx, c["r"]), dev(ctx, c["g"]), dev(ctx, c["b"])
    out = DeviceTensor(ctx, (rows, cols), np.float32)
    with launched(ctx) as k:
        ctx.call("rten_hip_add_layer_norm_f32", rows, cols, xd.vp, rd.vp, gd.vp, bd.vp, 1.0, 0.0, 1e-12, out.vp)
    assert k.names == {"add_layer_norm_f32"}, k.names
    same_bits(out.numpy(), c["added"], f"Add + LayerNorm {cols} columns, x {band}")


@pytest.mark.parametrize("inner,band", RC.INSTANCE_NORM_CASES)
def test_instance_norm_every_path(ctx, inner, band):
    c = RC.instance_norm_case(inner, band)
    for name, path in INSTANCE_NORM_PATHS.items():
        with launched(ctx) as k:
            got = run_instance_norm(ctx, c["x"], c["scale"], c["bias"], 1e-5, path)
        assert k.names == {"instance_norm_f32"}, k.names
        same_bits(got, c["want"], f"InstanceNorm inner {inner}, x {band}, path {name}")


# ------------------------------------------------------------------------------------------ pooling
def test_average_pools_of_subnormal_inputs(ctx):
    c = RC.pool_case()
    with launched(ctx) as k:
        for cip in (False, True):
            got = ops.AveragePool((3, 3), padding=[1, 1, 1, 1], strides=(2, 2), count_include_pad=cip).run(ctx, [dev(ctx, c["x"])])[0].numpy()
            same_bits(got, c["avg"][cip], f"AveragePool subnormal input count_include_pad={cip}")
        same_bits(ops.GlobalAveragePool().run(ctx, [dev(ctx, c["xg"])])[0].numpy(), c["gap"], "GlobalAveragePool subnormal input")
    assert "global_average_pool_f32" in k.names and any("average_pool" in n and n != "global_average_pool_f32" for n in k.names), k.names


# ------------------------------------------------------------------------------------------ GRU / LSTM
@pytest.mark.parametrize("lstm,direction,band", RC.RNN_CASES, ids=lambda v: {False: "gru", True: "lstm"}.get(v, v) if isinstance(v, bool) else v)
def test_rnn_composed_and_fused(ctx, lstm, direction, band):
    """rnn_tiny: h is subnormal when the fused kernel writes it to LDS and reads it back as the next step's MFMA operand."""
    c = RC.rnn_case(lstm, direction, band)
    name = "lstm" if lstm else "gru"
    for path, label, kernel in ((L.RNN_PATH_COMPOSED, "composed", f"{name}_gate_kernel"), (L.RNN_PATH_FUSED, "fused", f"{name}_fused_kernel")):
        with launched(ctx) as k:
            got = run_abi(ctx, lstm, c["t"], c["c"], path)
        assert kernel in k.names and (f"{name}_fused_kernel" in k.names) == (label == "fused"), k.names
        for out, want, which in zip(got, c["want"], ("Y", "Y_h", "Y_c")):
            same_bits(out, want, f"{name.upper()} {direction} {band} {label} path {which}")


# ------------------------------------------------------------------------------------------ MatMulNBits
@pytest.mark.parametrize("case", RC.NBITS_CASES, ids=lambda v: "-".join(map(str, v)))
def test_matmul_nbits_subnormal_and_overflowing_scales(ctx, case):
    """One row: the vector kernel, whose fma(q, s, -8 s) dequantisation holds only while 8 s is finite.  Four rows: the expansion kernel and the f32 GEMM."""
    rows, kk, bs, band = case
    c = RC.nbits_case(*case)
    with launched(ctx) as k:
        got = ops.MatMulNBits(4, bs).run(ctx, [dev(ctx, c["lhs"]), dev(ctx, c["quant"]), dev(ctx, c["scales"])])[0].numpy()
    assert ("gemv_f32_q4" in k.names) == (rows == 1) and ("dequant_q4" in k.names) == (rows > 1), k.names
    same_bits(got, c["want"], f"MatMulNBits rows {rows} K {kk} block {bs} {band}")


# ------------------------------------------------------------------------------------------ DynamicQuantizeLinear
@pytest.mark.parametrize("kind", RC.DQL_INPUTS)
def test_dynamic_quantize_linear(ctx, kind):
    c = RC.dql_case(kind, False)
    with launched(ctx) as k:
        y, s, z = ops.DynamicQuantizeLinear().run(ctx, [dev(ctx, c["x"])])
    assert "dynamic_quantize_linear" in k.names, k.names
    same_bits(s.numpy().reshape(1), np.array([c["scale"]], np.float32), f"DynamicQuantizeLinear {kind} scale")
    assert int(z.numpy()) == c["zero_point"], f"DynamicQuantizeLinear {kind} zero point: got {int(z.numpy())}, expected {c['zero_point']}"
    same_bits(y.numpy(), c["codes"], f"DynamicQuantizeLinear {kind} codes")


@pytest.mark.parametrize("kind", RC.DQL_INPUTS)
def test_dynamic_quantize_linear_staged(ctx, kind):
    """The staged form quantises straight into its consumer's padded 16-channel image; the image is rebuilt from the oracle's codes."""
    c = RC.dql_case(kind, True)
    N, Cc, H, W, O, ks, pad, stride = RC.DQL_STAGED_GEOM
    oh, ow = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    for pm in (L.PAD_ZERO_POINT, L.PAD_RAW0_I8):
        d = L.Conv2dInt8Desc(L.Conv2dDesc(N, Cc, H, W, O, ks, ks, (C.c_int32 * 4)(pad, pad, pad, pad), stride, stride, 1, 1, 1, oh, ow), 0, 1, 0, pm, 1, 1)
        staged = DeviceTensor(ctx, (ctx.lib.rten_hip_conv2d_int8_staged_bytes(C.byref(d)),), np.uint8)
        xd, xs, xz = dev(ctx, c["x"]), DeviceTensor(ctx, (1,), np.float32), DeviceTensor(ctx, (1,), np.uint8)
        with launched(ctx) as k:
            ctx.call("rten_hip_dynamic_quantize_linear_staged", C.byref(d), xd.vp, staged.vp, xs.vp, xz.vp, None, None)
        assert any(n.startswith("dynamic_quantize_linear_staged") for n in k.names), k.names
        same_bits(xs.numpy(), np.array([c["scale"]], np.float32), f"staged DynamicQuantizeLinear {kind} scale")
        assert int(xz.numpy()[0]) == c["zero_point"], f"staged DynamicQuantizeLinear {kind} zero point: got {int(xz.numpy()[0])}, expected {c['zero_point']}"
        want = staged_image(c["codes"], c["zero_point"], (pad,) * 4, pm)
        same_bits(staged.numpy()[:want.size], want, f"staged DynamicQuantizeLinear {kind} pad mode {pm} image")


# ------------------------------------------------------------------------------------------ ConvIntegerToFloat epilogue
@pytest.mark.parametrize("kind", RC.CI2F_CASES)
def test_conv_integer_to_float_epilogue(ctx, kind):
    """The operator tries the staged LDS-DMA kernel first and runs the generic one where that does not cover the call; each has a float epilogue of its own.
    Both are run (int8 path 0 = automatic, which covers this shape with the 64x128 tile that eight output channels select; 1 = generic only)."""
    c = RC.ci2f_case(kind)
    ins = [dev(ctx, c["x"]), dev(ctx, c["w"]), dev(ctx, c["x_zp"]), None, dev(ctx, c["scale"])]
    for path, kernel, other in ((0, "igemm_i8_fast_kernel<64,128>", "igemm_i8_kernel<"), (1, "igemm_i8_kernel<1>", "igemm_i8_fast_kernel<")):
        ctx.call("rten_hip_set_int8_path", path)
        try:
            with launched(ctx) as k:
                plain = ops.ConvIntegerToFloat(ops.ConvInteger()).run(ctx, ins)[0].numpy()
                biased = ops.ConvIntegerToFloat(ops.ConvInteger()).run(ctx, ins + [dev(ctx, c["bias"])])[0].numpy()
        finally:
            ctx.call("rten_hip_set_int8_path", 0)
        assert kernel in k.names and not k.ran(other), (path, k.names)
        same_bits(plain, c["plain"], f"ConvIntegerToFloat {kind} {kernel}")
        same_bits(biased, c["biased"], f"ConvIntegerToFloat {kind} {kernel} with bias")
