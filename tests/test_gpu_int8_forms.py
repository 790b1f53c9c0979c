"""The dispatch table of the fast int8 path (csrc/int8_fast.hip, `rten_i8_dispatch_fast`): every launch form that needs no process-level knob, under each of
the four tile settings of rten_hip_set_int8_tile.  Per combination one tiny convolution runs, its outputs are compared bit for bit with the CPU oracle, and the
kernel label the launch was profiled under is asserted -- plans, tools and other tests match on those labels.

Shapes: N = 1, 8x8 output, O = 64, so every tile setting gives one workgroup.  `c64_1x1` has one k-tile; `c128_3x3` has Kp = 9 * 128 = 1152 = 18 k-tiles, which is
at least 16 on an under-filled launch, so tile setting 3 takes the 64x64 kernel with four k-groups and the label says `kg4` (forms built with k-groups only).
The cross-workgroup K split needs RTEN_I8_KS in the environment: tests/test_gpu_round6.py runs it in a child process."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import ref
from rten_amd import lib as L
from rten_amd.tensor import DeviceTensor
from tests.test_gpu_range import launched
from tests.test_gpu_round3 import _conv_desc, bits_equal, dev, staged_image

pytestmark = pytest.mark.gpu

N, HW, O = 1, 8, 64
CASES = {"c64_1x1": (64, 1, 0), "c128_3x3": (128, 3, 1)}  # input channels, kernel size, padding (stride 1: the output is 8x8 as well)
TILE_NAMES = ("128,128", "128,64", "64,128", "64,64")
KERNEL = "igemm_i8_fast_kernel<"
NEXT_PAD_MODE = L.PAD_ZERO_POINT  # the consumer of the quantized-output forms: 3x3, padding 1, border = its input's zero point


def tile_name(case, tile, k_groups):
    c, k, _ = CASES[case]
    nkt = -(-(k * k * c) // 64)  # (C is a multiple of 16: no channel padding)
    return TILE_NAMES[tile] + (",kg4" if k_groups and tile == 3 and nkt >= 16 else "")


def fast_kernels(k):
    return {n for n in k.names if n.startswith(KERNEL)}


@functools.lru_cache(maxsize=None)
def problem(case):
    """Host data of one case and everything the oracle says about it (computed once, read by every test)."""
    c, k, pad = CASES[case]
    rng = ref.XorShiftRng(977 + c)
    p = {"xf": (rng.f32(N * c * HW * HW).reshape(N, c, HW, HW) - 0.3).astype(np.float32), "wq": rng.i8(O * c * k * k, reduced=True).reshape(O, c, k, k),
         "ws": (rng.f32(1) * 0.01 + 0.002).astype(np.float32), "bias": rng.f32(O) - 0.5, "res": rng.f32(N * O * HW * HW).reshape(N, O, HW, HW) - 0.5}
    # DynamicQuantizeLinear -> ConvInteger -> Cast -> Mul -> Add(bias) [-> Add(residual)] -> Relu, in the reference's operator order
    p["q"], p["s"], p["z"] = ref.dynamic_quantize_linear(p["xf"])
    acc = ref.conv2d_int8(p["q"], p["wq"], x_zp=int(p["z"]), pads=(pad,) * 4, pad_mode=L.PAD_RAW0_I8)
    y = acc.astype(np.float32) * (p["ws"] * np.float32(p["s"])).astype(np.float32)[0] + p["bias"][None, :, None, None]
    p["y"], p["y_res"] = ref.relu(y.astype(np.float32)), ref.relu((y + p["res"]).astype(np.float32))
    # ... and the DynamicQuantizeLinear of the one consumer of y: its codes, laid out as the consumer's staged image, and its scale product
    p["q2"], p["s2"], p["z2"] = ref.dynamic_quantize_linear(p["y"])
    p["ws2"] = np.array([0.0173], np.float32)
    p["image2"] = staged_image(p["q2"], p["z2"], (1,) * 4, NEXT_PAD_MODE)
    # ... and the pointwise convolution that quantizes y in its loader (with residual and Relu)
    p["wq3"] = rng.i8(O * O, reduced=True).reshape(O, O, 1, 1)
    acc3 = ref.conv2d_int8(p["q2"], p["wq3"], x_zp=int(p["z2"]), pad_mode=L.PAD_RAW0_I8)
    y3 = acc3.astype(np.float32) * (p["ws2"] * np.float32(p["s2"])).astype(np.float32)[0] + p["bias"][None, :, None, None] + p["res"]
    p["y3"] = ref.relu(y3.astype(np.float32))
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


def each_tile(ctx, run):
    """run(tile) under each tile setting; the per-shape rule is restored whatever happens."""
    try:
        for tile in range(4):
            ctx.call("rten_hip_set_int8_tile", tile, None)
            run(tile)
    finally:
        ctx.call("rten_hip_set_int8_tile", -1, None)


@pytest.mark.parametrize("with_res", (False, True), ids=("plain", "residual"))
@pytest.mark.parametrize("case", CASES)
def test_plain_form(ctx, case, with_res):
    """Raw u8 activations and i8 weights: the entry point stages both, then launches the plain form (the residual changes the kernel, not its label)."""
    p, (c, k, pad) = problem(case), CASES[case]
    d, _, _ = _conv_desc(N, c, HW, HW, O, k, 1, pad, packed=0, staged=0)
    x, w, z, sc, bias, res = (dev(ctx, a) for a in (p["q"], p["wq"], np.array([p["z"]], np.uint8), p["ws"] * np.float32(p["s"]), p["bias"], p["res"]))

    def run(tile):
        y = dev(ctx, np.zeros((N, O, HW, HW), np.float32))
        with launched(ctx) as kn:
            ctx.call("rten_hip_conv2d_int8", C.byref(d), x.vp, w.vp, z.vp, None, sc.vp, bias.vp, res.vp if with_res else None,
                     L.CONV_RELU | (L.CONV_RESIDUAL if with_res else 0), y.vp)
        assert fast_kernels(kn) == {f"{KERNEL}{tile_name(case, tile, True)}>"}, (tile, kn.names)
        bits_equal(y.numpy(), p["y_res"] if with_res else p["y"])

    each_tile(ctx, run)


def staged_producer(ctx, case):
    """The operands the quantized-output forms need: the input quantized into its staged image, prepacked weights, the combined scale."""
    p, (c, k, pad) = problem(case), CASES[case]
    d, _, _ = _conv_desc(N, c, HW, HW, O, k, 1, pad)
    staged = DeviceTensor(ctx, (ctx.lib.rten_hip_conv2d_int8_staged_bytes(C.byref(d)),), np.uint8)
    packed = DeviceTensor(ctx, (ctx.lib.rten_hip_conv2d_int8_packed_bytes(C.byref(d)),), np.uint8)
    xs, xz, sc = DeviceTensor(ctx, (1,), np.float32), DeviceTensor(ctx, (1,), np.uint8), DeviceTensor(ctx, (1,), np.float32)
    xf, wq, ws = dev(ctx, p["xf"]), dev(ctx, p["wq"]), dev(ctx, p["ws"])
    ctx.call("rten_hip_dynamic_quantize_linear_staged", C.byref(d), xf.vp, staged.vp, xs.vp, xz.vp, None, None)
    ctx.call("rten_hip_mul_f32", 1, ws.vp, xs.vp, 1, sc.vp)
    ctx.call("rten_hip_conv2d_int8_prepack", C.byref(d), wq.vp, packed.vp)
    ctx.sync()
    assert xs.numpy()[0] == p["s"] and xz.numpy()[0] == p["z"]
    return d, staged, packed, xz, sc


@pytest.mark.parametrize("form", ("exchange", "recompute"))
@pytest.mark.parametrize("case", CASES)
def test_quantized_output_forms(ctx, case, form):
    """rten_hip_conv2d_int8_qout with an exchange block (one launch) and with sync == NULL (a statistics pass under the plain label, then the convolution again):
    the f32 output, the consumer's staged image (border included), its scale, zero point and scale product, against the oracle."""
    p, lib = problem(case), ctx.lib
    d, staged, packed, xz, sc = staged_producer(ctx, case)
    d2, _, _ = _conv_desc(N, O, HW, HW, 64, 3, 1, 1, pad_mode=NEXT_PAD_MODE)
    bias, ws2 = dev(ctx, p["bias"]), dev(ctx, p["ws2"])
    sync = None
    if form == "exchange":
        sync = DeviceTensor(ctx, (lib.rten_hip_grid_sync_bytes(),), np.uint8)
        ctx.call("rten_hip_grid_sync_reset", sync.vp, 1)
    nb = lib.rten_hip_conv2d_int8_staged_bytes(C.byref(d2))
    assert nb >= p["image2"].size

    def run(tile):
        stats = DeviceTensor(ctx, (lib.rten_hip_minmax_stats_bytes(),), np.uint8)
        ctx.call("rten_hip_minmax_stats_reset", stats.vp, 1)
        image, y = dev(ctx, np.full(nb, 0xEE, np.uint8)), dev(ctx, np.zeros((N, O, HW, HW), np.float32))
        s2, z2, pr = DeviceTensor(ctx, (1,), np.float32), DeviceTensor(ctx, (1,), np.uint8), DeviceTensor(ctx, (1,), np.float32)
        with launched(ctx) as kn:
            ctx.call("rten_hip_conv2d_int8_qout", C.byref(d), staged.vp, packed.vp, xz.vp, None, sc.vp, bias.vp, None, L.CONV_RELU, y.vp, stats.vp,
                     sync.vp if sync else None, C.byref(d2), image.vp, s2.vp, z2.vp, ws2.vp, pr.vp)
        name = tile_name(case, tile, True)
        want = {f"{KERNEL}{name},qo>"} if sync else {f"{KERNEL}{name}>", f"{KERNEL}{name},qo2>"}
        assert fast_kernels(kn) == want, (tile, kn.names)
        if sync:
            timeouts = C.c_int32(-1)
            ctx.call("rten_hip_grid_sync_timeouts", sync.vp, 1, C.byref(timeouts))
            assert timeouts.value == 0, "the launch gave up waiting for its grid"
        bits_equal(y.numpy(), p["y"])
        assert np.array_equal(image.numpy()[:p["image2"].size], p["image2"]), (tile, "the consumer's staged image differs from the oracle's codes")
        assert s2.numpy()[0] == p["s2"] and z2.numpy()[0] == p["z2"] and pr.numpy()[0] == np.float32(np.float32(p["s2"]) * p["ws2"][0]), tile

    each_tile(ctx, run)


def test_quantize_on_load_form(ctx):
    """rten_hip_conv2d_int8_dql on the f32 output of the 1x1 case and the statistics its producer left (pointwise, C % 64 == 0: the form's whole domain; it
    is built with one k-group on every tile)."""
    p, lib = problem("c64_1x1"), ctx.lib
    sb = lib.rten_hip_minmax_stats_bytes()
    # the producer: the plain form with a statistics block; its output is the oracle's, so the consumer below is compared with the oracle alone
    d0, _, _ = _conv_desc(N, 64, HW, HW, O, 1, 1, 0, packed=0, staged=0)
    x, w, z, sc, bias, res = (dev(ctx, a) for a in (p["q"], p["wq"], np.array([p["z"]], np.uint8), p["ws"] * np.float32(p["s"]), p["bias"], p["res"]))
    t, in_stats = DeviceTensor(ctx, (N, O, HW, HW), np.float32), DeviceTensor(ctx, (sb,), np.uint8)
    ctx.call("rten_hip_minmax_stats_reset", in_stats.vp, 1)
    ctx.call("rten_hip_conv2d_int8_stats", C.byref(d0), x.vp, w.vp, z.vp, None, sc.vp, bias.vp, None, L.CONV_RELU, t.vp, in_stats.vp)
    ctx.sync()
    bits_equal(t.numpy(), p["y"])
    d, _, _ = _conv_desc(N, O, HW, HW, O, 1, 1, 0)
    packed = DeviceTensor(ctx, (lib.rten_hip_conv2d_int8_packed_bytes(C.byref(d)),), np.uint8)
    wq3, ws2 = dev(ctx, p["wq3"]), dev(ctx, p["ws2"])
    ctx.call("rten_hip_conv2d_int8_prepack", C.byref(d), wq3.vp, packed.vp)

    def run(tile):
        y, out_stats = dev(ctx, np.zeros((N, O, HW, HW), np.float32)), DeviceTensor(ctx, (sb,), np.uint8)
        ctx.call("rten_hip_minmax_stats_reset", out_stats.vp, 1)
        xs, xz = DeviceTensor(ctx, (1,), np.float32), DeviceTensor(ctx, (1,), np.uint8)
        with launched(ctx) as kn:
            ctx.call("rten_hip_conv2d_int8_dql", C.byref(d), t.vp, in_stats.vp, packed.vp, ws2.vp, bias.vp, res.vp, L.CONV_RELU | L.CONV_RESIDUAL, y.vp,
                     out_stats.vp, xs.vp, xz.vp)
        assert fast_kernels(kn) == {f"{KERNEL}{tile_name('c64_1x1', tile, False)},bq>"}, (tile, kn.names)
        bits_equal(y.numpy(), p["y3"])
        assert xs.numpy()[0] == p["s2"] and xz.numpy()[0] == p["z2"], tile

    each_tile(ctx, run)
