#!/usr/bin/env python3
"""Per-kernel microbench: every hot-path kernel class of SURVEY.md section 8 against the roofline that bounds it.

Not the driver's contract (that is bench.py); this writes one JSON document with a row per kernel:
    {"op": ..., "shape": ..., "us": ..., "bound": "hbm"|"mfma", "achieved": ..., "unit": "GB/s"|"TFLOP/s", "frac": ...}
Sizes are the ones the BASELINE configs put on these kernels (ResNet-50 batch 32, BERT-base batch 32 x 128).

    python tools/bench_ops.py [--reps 20] > gpurun_out/ops.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rten_amd import lib as L  # noqa: E402
from rten_amd.tensor import DeviceTensor  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: 8 TB/s spec (about 6.3 TB/s achievable)
F32_PEAK_TF = 157.3     # v_mfma_f32_32x32x2_f32, 256 CUs x 2.4 GHz
I8_PEAK_TOPS = 5033.0   # v_mfma_i32_32x32x32_i8: 32768 MAC / 16 cycles per CU -> 256 CUs x 2.4 GHz (dense)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="", help="substring filter on the op name (e.g. Integer)")
    ap.add_argument("--cpu-baseline", action="store_true", help="add bench.py's CPU-oracle timing (cpu_baseline leg) beside every row")
    args = ap.parse_args()
    ctx = L.Context(0)
    rng = np.random.default_rng(0)
    rows = []

    def dev(a):
        return DeviceTensor.from_numpy(ctx, np.ascontiguousarray(a))

    def empty(shape, dt=np.float32):
        return DeviceTensor(ctx, shape, dt)

    def timeit(fn):
        # warm the clocks on THIS kernel first (the chip re-clocks within tens of milliseconds of a change of load; a cold
        # first batch reads 10-15 % slow on the MFMA rows), then keep the best of three timed batches
        import time
        fn()
        ctx.sync()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.03:
            for _ in range(args.reps):
                fn()
            ctx.sync()
        best = 1e30
        for _ in range(3):
            ctx.timer_start(3)
            for _ in range(args.reps):
                fn()
            ctx.timer_stop(3)
            best = min(best, ctx.timer_ms(3) / args.reps * 1e3)
        return best  # us

    def want(op):
        return args.only.lower() in op.lower()

    def hbm(op, shape, fn, nbytes):
        if not want(op):
            return
        us = timeit(fn)
        gbs = nbytes / us / 1e3
        rows.append({"op": op, "shape": shape, "us": round(us, 2), "bound": "hbm", "achieved": round(gbs, 1), "unit": "GB/s",
                     "peak": HBM_PEAK_GBS, "frac": round(gbs / HBM_PEAK_GBS, 3), "algorithmic_bytes": int(nbytes)})

    def mfma(op, shape, fn, flops, peak, unit):
        if not want(op):
            return
        us = timeit(fn)
        t = flops / us / 1e6
        rows.append({"op": op, "shape": shape, "us": round(us, 2), "bound": "mfma", "achieved": round(t, 2), "unit": unit,
                     "peak": peak, "frac": round(t / peak, 3), "algorithmic_ops": int(flops)})

    # ---- element-wise / row-wise kernels on ResNet stage-0 and BERT activations
    n_act = 32 * 256 * 56 * 56
    x = dev(rng.standard_normal(n_act, dtype=np.float32))
    x2 = dev(rng.standard_normal(n_act, dtype=np.float32))
    y = empty((n_act,))
    hbm("Relu", f"n={n_act}", (lambda: ctx.call("rten_hip_relu_f32", n_act, x.vp, y.vp)), 8.0 * n_act)
    hbm("Add", f"n={n_act}", (lambda: ctx.call("rten_hip_add_f32", n_act, x.vp, x2.vp, n_act, y.vp)), 12.0 * n_act)
    n_ffn = 4096 * 3072
    hbm("Gelu", f"n={n_ffn}", (lambda: ctx.call("rten_hip_gelu_f32", n_ffn, x.vp, y.vp)), 8.0 * n_ffn)
    hbm("Erf", f"n={n_ffn}", (lambda: ctx.call("rten_hip_erf_f32", n_ffn, x.vp, y.vp)), 8.0 * n_ffn)
    # the parameterised activation kernel, every kind, at 12.6 M elements (rten_hip_activation_f32)
    for name, kind, a, b in (("Sigmoid", L.ACT_SIGMOID, 0.0, 0.0), ("Silu", L.ACT_SILU, 0.0, 0.0), ("Swish", L.ACT_SWISH, 1.702, 0.0),
                             ("HardSigmoid", L.ACT_HARD_SIGMOID, 0.2, 0.5), ("HardSwish", L.ACT_HARD_SWISH, 0.0, 0.0), ("Clip", L.ACT_CLIP, 0.0, 6.0),
                             ("LeakyRelu", L.ACT_LEAKY_RELU, 0.01, 0.0), ("Elu", L.ACT_ELU, 1.0, 0.0)):
        hbm(f"activation {name}", f"n={n_ffn}", (lambda kind=kind, a=a, b=b: ctx.call("rten_hip_activation_f32", kind, a, b, n_ffn, x.vp, y.vp)), 8.0 * n_ffn)
    r, c = 32 * 12 * 128, 128
    hbm("Softmax", f"rows={r} cols={c}", (lambda: ctx.call("rten_hip_softmax_f32", r, c, x.vp, None, 1, 1, 0, y.vp)), 8.0 * r * c)
    r, c = 4096, 768
    g, b = dev(np.ones(c, np.float32)), dev(np.zeros(c, np.float32))
    hbm("LayerNormalization", f"rows={r} cols={c}",
        (lambda: ctx.call("rten_hip_layer_norm_f32", r, c, x.vp, g.vp, b.vp, C.c_float(1.0), C.c_float(0.0), C.c_float(1e-12), y.vp)), 8.0 * r * c)
    # reference point for the short row-wise launches: a device copy of the same 12.6 MB (the fraction of the HBM peak ANY 6 us launch can
    # reach is bounded by its ramp-up and drain; LayerNormalization is to be read against this row, not against 8 TB/s)
    hbm("copy, LayerNormalization's size (reference point)", f"{4 * r * c} B", (lambda: ctx.call("rten_hip_memcpy_d2d", y.vp, x.vp, C.c_size_t(4 * r * c))), 8.0 * r * c)
    u8 = empty((n_act,), np.uint8)
    sc, zp = empty((1,)), empty((1,), np.uint8)
    hbm("DynamicQuantizeLinear", f"n={n_act}", (lambda: ctx.call("rten_hip_dynamic_quantize_linear", n_act, x.vp, u8.vp, sc.vp, zp.vp)), 9.0 * n_act)
    xi = dev(rng.integers(-1000, 1000, n_act).astype(np.int32))
    hbm("cast_scale", f"n={n_act}", (lambda: ctx.call("rten_hip_cast_scale", n_act, xi.vp, sc.vp, 1, y.vp)), 8.0 * n_act)
    pd = L.Pool2dDesc(32, 64, 112, 112, 3, 3, 2, 2, (C.c_int32 * 4)(1, 1, 1, 1), 56, 56, 0)
    n_in, n_out = 32 * 64 * 112 * 112, 32 * 64 * 56 * 56
    hbm("MaxPool 3x3/2", "32x64x112x112", (lambda: ctx.call("rten_hip_max_pool2d_f32", C.byref(pd), x.vp, y.vp)), 4.0 * (n_in + n_out))
    st = empty((ctx.lib.rten_hip_minmax_stats_bytes(),), np.uint8)
    ctx.call("rten_hip_minmax_stats_reset", st.vp, 1)
    hbm("MaxPool 3x3/2 + statistics for the following DynamicQuantizeLinear", "32x64x112x112",
        (lambda: ctx.call("rten_hip_max_pool2d_f32_stats", C.byref(pd), x.vp, y.vp, st.vp)), 4.0 * (n_in + n_out))
    hbm("GlobalAveragePool", "32x2048x7x7", (lambda: ctx.call("rten_hip_global_average_pool_f32", 32 * 2048, 49, x.vp, y.vp)), 4.0 * 32 * 2048 * 50)

    # InstanceNormalization (few, long slices) on every path, BatchNormalization with a fused activation, LogSoftmax -- each beside a device copy of the
    # same bytes (the rate a launch of that size can reach at all)
    def copy_row(what, n_el):
        hbm(f"copy, {what} (reference point)", f"{4 * n_el} B", (lambda: ctx.call("rten_hip_memcpy_d2d", y.vp, x.vp, C.c_size_t(4 * n_el))), 8.0 * n_el)

    for n, c, h, w in ((8, 64, 128, 128), (1, 32, 512, 512), (32, 256, 32, 32)):
        sc_c, bi_c = dev(rng.standard_normal(c, dtype=np.float32)), dev(rng.standard_normal(c, dtype=np.float32))
        for pname, path in (("streaming", L.INSTANCE_NORM_PATH_STREAMING), ("resident", L.INSTANCE_NORM_PATH_RESIDENT), ("auto", L.INSTANCE_NORM_PATH_AUTO)):
            if want("InstanceNormalization"):
                ctx.call("rten_hip_set_instance_norm_path", path)
            hbm(f"InstanceNormalization ({pname})", f"{n}x{c}x{h}x{w}",
                (lambda n=n, c=c, h=h, w=w, sc_c=sc_c, bi_c=bi_c: ctx.call("rten_hip_instance_norm_f32", n, c, h * w, x.vp, sc_c.vp, bi_c.vp, 1e-5, L.ACT_RELU, 0.0, 0.0, y.vp)),
                8.0 * n * c * h * w)
        ctx.call("rten_hip_set_instance_norm_path", L.INSTANCE_NORM_PATH_AUTO)
        copy_row(f"InstanceNormalization {n}x{c}x{h}x{w}", n * c * h * w)
    bn_c = 256
    bn_p = [dev(np.abs(rng.standard_normal(bn_c, dtype=np.float32)) + 0.5) for _ in range(4)]
    hbm("batch_norm_f32_act (Relu)", "32x256x56x56",
        (lambda: ctx.call("rten_hip_batch_norm_f32_act", 32, bn_c, 56 * 56, x.vp, *[t.vp for t in bn_p], 1e-5, L.ACT_RELU, 0.0, 0.0, y.vp)), 8.0 * n_act)
    hbm("batch_norm_f32", "32x256x56x56", (lambda: ctx.call("rten_hip_batch_norm_f32", 32, bn_c, 56 * 56, x.vp, *[t.vp for t in bn_p], 1e-5, y.vp)), 8.0 * n_act)
    copy_row("batch_norm 32x256x56x56", n_act)
    for r, c in ((4096, 97), (64, 32000)):
        hbm("LogSoftmax", f"rows={r} cols={c}", (lambda r=r, c=c: ctx.call("rten_hip_log_softmax_f32", r, c, x.vp, y.vp)), 8.0 * r * c)
        copy_row(f"LogSoftmax {r}x{c}", r * c)

    # Unary math, Pow, Max and Pad at 32x64x56x56 (--only math: selects these rows), beside the parameterised activation kernel's Sigmoid at the same element count (the row they are read
    # against: same bytes, more arithmetic).  Positive operands, so that Log / Pow(0.5) / Softplus run their ordinary path.
    mshape = (32, 64, 56, 56)
    n_m = int(np.prod(mshape))
    xp = dev(np.abs(rng.standard_normal(n_m, dtype=np.float32)) + np.float32(0.1))
    hbm("math: activation Sigmoid (reference point)", f"n={n_m}", (lambda: ctx.call("rten_hip_activation_f32", L.ACT_SIGMOID, 0.0, 0.0, n_m, xp.vp, y.vp)), 8.0 * n_m)
    for name, code in (("Exp", L.UNARY_EXP), ("Log", L.UNARY_LOG), ("Sqrt", L.UNARY_SQRT), ("Neg", L.UNARY_NEG), ("Softplus", L.UNARY_SOFTPLUS)):
        hbm(f"math: unary {name}", f"n={n_m}", (lambda code=code: ctx.call("rten_hip_unary_f32", code, n_m, xp.vp, y.vp)), 8.0 * n_m)
    i64 = lambda v: (C.c_int64 * len(v))(*v)
    dense, zero = i64([64 * 56 * 56, 56 * 56, 56, 1]), i64([0, 0, 0, 0])
    for e in (2.0, 0.5):
        ed = dev(np.array(e, np.float32))
        hbm(f"math: Pow({e:g})", "32x64x56x56 x []", (lambda ed=ed: ctx.call("rten_hip_binary_broadcast_f32", L.BINARY_POW, 4, i64(mshape), dense, zero, xp.vp, ed.vp, y.vp)), 8.0 * n_m)
    hbm("math: Max (two operands)", "32x64x56x56 x 32x64x56x56", (lambda: ctx.call("rten_hip_binary_broadcast_f32", L.BINARY_MAX, 4, i64(mshape), dense, dense, xp.vp, x2.vp, y.vp)), 12.0 * n_m)
    n_pad = 32 * 64 * 58 * 58
    for mname, mode in (("reflect", L.PAD_REFLECT), ("constant", L.PAD_CONSTANT)):
        hbm(f"math: Pad {mname} by 1", "32x64x56x56 -> 32x64x58x58", (lambda mode=mode: ctx.call("rten_hip_pad_b32", mode, 4, i64(mshape), i64([0, 0, 1, 1, 0, 0, 1, 1]), 0, xp.vp, y.vp)),
            4.0 * (n_m + n_pad))

    # QuantizeLinear / DequantizeLinear at the shape of the math rows (--only qdq: selects these rows): per-tensor u8, the fused round trip beside the two
    # launches it replaces, and the per-axis (axis 1: 64 channels of 56 x 56) forms.  The Sigmoid row is measured before and after the others: the round trip moves
    # the same 8 bytes per element with less arithmetic, and the two readings of that row give the spread it is read against.
    xq_in = dev((rng.standard_normal(n_m, dtype=np.float32) * np.float32(2.0)))
    q8 = empty((n_m,), np.uint8)
    s1, z1 = dev(np.array(0.05, np.float32)), dev(np.array(128, np.uint8))
    s64, z64 = dev(np.linspace(0.02, 0.08, 64).astype(np.float32)), dev(np.arange(96, 160, dtype=np.uint8))
    per_tensor, per_axis = (1, 1, n_m), (32, 64, 56 * 56)
    sigmoid_row = lambda tag: hbm(f"qdq: activation Sigmoid (reference point, {tag})", f"n={n_m}", (lambda: ctx.call("rten_hip_activation_f32", L.ACT_SIGMOID, 0.0, 0.0, n_m, xq_in.vp, y.vp)), 8.0 * n_m)
    quant = lambda g, s, z: ctx.call("rten_hip_quantize_linear_f32", L.DT_U8, *g, xq_in.vp, s.vp, z.vp, q8.vp)
    dequant = lambda g, s, z: ctx.call("rten_hip_dequantize_linear_f32", L.DT_U8, *g, q8.vp, s.vp, z.vp, y.vp)
    fused = lambda g, s, z: ctx.call("rten_hip_quantize_dequantize_f32", L.DT_U8, *g, xq_in.vp, s.vp, z.vp, y.vp)
    sigmoid_row("first")
    hbm("qdq: quantize u8, per-tensor", "32x64x56x56", (lambda: quant(per_tensor, s1, z1)), 5.0 * n_m)
    hbm("qdq: dequantize u8, per-tensor", "32x64x56x56", (lambda: dequant(per_tensor, s1, z1)), 5.0 * n_m)
    hbm("qdq: round trip u8, per-tensor, one launch", "32x64x56x56", (lambda: fused(per_tensor, s1, z1)), 8.0 * n_m)
    hbm("qdq: quantize + dequantize u8, per-tensor, two launches", "32x64x56x56", (lambda: (quant(per_tensor, s1, z1), dequant(per_tensor, s1, z1))), 10.0 * n_m)
    hbm("qdq: quantize u8, per-axis (axis 1)", "32x64x56x56", (lambda: quant(per_axis, s64, z64)), 5.0 * n_m)
    hbm("qdq: round trip u8, per-axis (axis 1), one launch", "32x64x56x56", (lambda: fused(per_axis, s64, z64)), 8.0 * n_m)
    sigmoid_row("second")

    # depthwise 3x3 (MobileNet-style: 32 x 144 x 56 x 56) and a 2x upsampling ConvTranspose (32 x 64 x 28 x 28 -> 32 x 32 x 56 x 56, 4x4 / 2)
    cdw = 144
    xdw, wdw, bdw = dev(rng.standard_normal((32, cdw, 56, 56), dtype=np.float32)), dev(rng.standard_normal((cdw, 1, 3, 3), dtype=np.float32)), dev(np.zeros(cdw, np.float32))
    ydw = empty((32, cdw, 56, 56))
    ddw = L.Conv2dDesc(32, cdw, 56, 56, cdw, 3, 3, (C.c_int32 * 4)(1, 1, 1, 1), 1, 1, 1, 1, cdw, 56, 56)
    hbm("Conv depthwise 3x3", f"32x{cdw}x56x56", (lambda: ctx.call("rten_hip_conv2d_f32", C.byref(ddw), xdw.vp, wdw.vp, 0, bdw.vp, None, 0, ydw.vp)), 8.0 * 32 * cdw * 56 * 56)
    # fused activation epilogue vs the same convolution with none, and vs convolution + the standalone kernel: the depthwise 3x3 above and a
    # MobileNet pointwise convolution (32 x 96 x 112 x 112 -> 24)
    ndw = 32 * cdw * 56 * 56
    hbm("Conv depthwise 3x3 + Clip(0, 6) fused", f"32x{cdw}x56x56",
        (lambda: ctx.call("rten_hip_conv2d_f32_act", C.byref(ddw), xdw.vp, wdw.vp, 0, bdw.vp, None, 0, L.ACT_CLIP, 0.0, 6.0, ydw.vp)), 8.0 * ndw)
    hbm("Conv depthwise 3x3 + Silu fused", f"32x{cdw}x56x56",
        (lambda: ctx.call("rten_hip_conv2d_f32_act", C.byref(ddw), xdw.vp, wdw.vp, 0, bdw.vp, None, 0, L.ACT_SILU, 0.0, 0.0, ydw.vp)), 8.0 * ndw)
    hbm("Conv depthwise 3x3, then standalone Silu", f"32x{cdw}x56x56",
        (lambda: (ctx.call("rten_hip_conv2d_f32", C.byref(ddw), xdw.vp, wdw.vp, 0, bdw.vp, None, 0, ydw.vp),
                  ctx.call("rten_hip_activation_f32", L.ACT_SILU, 0.0, 0.0, ndw, ydw.vp, ydw.vp))), 8.0 * ndw)
    dpw = L.Conv2dDesc(32, 96, 112, 112, 24, 1, 1, (C.c_int32 * 4)(0, 0, 0, 0), 1, 1, 1, 1, 1, 112, 112)
    xpw, bpw = dev(rng.standard_normal((32, 96, 112, 112), dtype=np.float32)), dev(np.zeros(24, np.float32))
    wpw = empty((ctx.lib.rten_hip_conv2d_f32_packed_bytes(C.byref(dpw)) // 4,))
    ctx.call("rten_hip_conv2d_f32_prepack", C.byref(dpw), dev(rng.standard_normal((24, 96, 1, 1), dtype=np.float32)).vp, wpw.vp)
    ypw = empty((32, 24, 112, 112))
    npw_in, npw_out = 32 * 96 * 112 * 112, 32 * 24 * 112 * 112
    for label, kind, a, b in (("no activation", L.ACT_NONE, 0.0, 0.0), ("+ Clip(0, 6) fused", L.ACT_CLIP, 0.0, 6.0), ("+ Silu fused", L.ACT_SILU, 0.0, 0.0)):
        hbm(f"Conv pointwise {label}", "32x96x112x112 -> 24",
            (lambda kind=kind, a=a, b=b: ctx.call("rten_hip_conv2d_f32_act", C.byref(dpw), xpw.vp, wpw.vp, 1, bpw.vp, None, 0, kind, a, b, ypw.vp)),
            4.0 * (npw_in + npw_out))
    hbm("Conv pointwise, then standalone Silu", "32x96x112x112 -> 24",
        (lambda: (ctx.call("rten_hip_conv2d_f32", C.byref(dpw), xpw.vp, wpw.vp, 1, bpw.vp, None, 0, ypw.vp),
                  ctx.call("rten_hip_activation_f32", L.ACT_SILU, 0.0, 0.0, npw_out, ypw.vp, ypw.vp))), 4.0 * (npw_in + npw_out))
    # Resize (rten_hip_resize_f32) at the sizes detectors and segmenters run it: YOLO's nearest 2x upsamplings at batch 32, a bilinear 2x
    # upsampling, DeepLab's logit upsampling (65 -> 513, pytorch_half_pixel); each beside a device copy that moves the same bytes (in + out)
    for label, (n_, c_, h_, w_), (oh_, ow_), mode, coord in (
            ("Resize nearest 2x", (32, 256, 40, 40), (80, 80), L.RESIZE_MODE_NEAREST, L.RESIZE_COORD_ASYMMETRIC),
            ("Resize nearest 2x", (32, 512, 20, 20), (40, 40), L.RESIZE_MODE_NEAREST, L.RESIZE_COORD_ASYMMETRIC),
            ("Resize linear half_pixel 2x", (32, 256, 64, 64), (128, 128), L.RESIZE_MODE_LINEAR, L.RESIZE_COORD_HALF_PIXEL),
            ("Resize linear pytorch_half_pixel (DeepLab logits)", (8, 21, 65, 65), (513, 513), L.RESIZE_MODE_LINEAR, L.RESIZE_COORD_PYTORCH_HALF_PIXEL)):
        if not want(label) and not want("copy, " + label):
            continue
        n_in, n_out = n_ * c_ * h_ * w_, n_ * c_ * oh_ * ow_
        xr, yr = dev(rng.standard_normal(n_in, dtype=np.float32)), empty((n_out,))
        shape = f"{n_}x{c_}x{h_}x{w_} -> {oh_}x{ow_}"
        hbm(label, shape, (lambda xr=xr, yr=yr, n_=n_, c_=c_, h_=h_, w_=w_, oh_=oh_, ow_=ow_, mode=mode, coord=coord: ctx.call(
            "rten_hip_resize_f32", mode, coord, L.RESIZE_NEAREST_FLOOR, n_ * c_, h_, w_, oh_, ow_, h_ / oh_, w_ / ow_, xr.vp, yr.vp)), 4.0 * (n_in + n_out))
        half = 2 * (n_in + n_out)  # bytes copied: read + write = the resize's input + output bytes
        del xr
        src = empty((half // 4,))
        hbm(f"copy, {label} (reference point)", f"{half} B", (lambda src=src, yr=yr, half=half: ctx.call("rten_hip_memcpy_d2d", yr.vp, src.vp, C.c_size_t(half))),
            4.0 * (n_in + n_out))
        del src, yr
    # the SwiGLU gate projection of a decoder MLP: 4096 x 768 x 3072 with Silu in the epilogue
    xs, ws = dev(rng.standard_normal((4096, 768), dtype=np.float32)), dev(rng.standard_normal((768, 3072), dtype=np.float32))
    ys = empty((4096, 3072))
    gsd = L.gemm_desc(4096, 3072, 768, 768, 1, 3072, 1, 3072)
    mfma("FusedMatMul+Silu", "4096x768x3072", (lambda: ctx.call("rten_hip_gemm_f32_act", C.byref(gsd), xs.vp, ws.vp, None, L.ACT_SILU, 0.0, 0.0, ys.vp)),
         2.0 * 4096 * 768 * 3072, F32_PEAK_TF, "TFLOP/s")
    mfma("MatMul (no activation, same shape)", "4096x768x3072", (lambda: ctx.call("rten_hip_gemm_f32", C.byref(gsd), xs.vp, ws.vp, None, ys.vp)),
         2.0 * 4096 * 768 * 3072, F32_PEAK_TF, "TFLOP/s")
    xct, wct, bct = dev(rng.standard_normal((32, 64, 28, 28), dtype=np.float32)), dev(rng.standard_normal((64, 32, 4, 4), dtype=np.float32)), dev(np.zeros(32, np.float32))
    yct = empty((32, 32, 56, 56))
    dct = L.Conv2dDesc(32, 64, 28, 28, 32, 4, 4, (C.c_int32 * 4)(1, 1, 1, 1), 2, 2, 1, 1, 1, 56, 56)
    mfma("ConvTranspose 4x4/2", "32x64x28x28 -> 32", (lambda: ctx.call("rten_hip_conv_transpose2d_f32", C.byref(dct), xct.vp, wct.vp, bct.vp, yct.vp)),
         2.0 * 32 * 64 * 28 * 28 * 32 * 16, F32_PEAK_TF, "TFLOP/s")

    # ---- MatMulNBits on LLM-decoder projections (4-bit blocks of 32): decode (1 row, bound by streaming the packed weights) on a
    # 4096 x 4096 attention projection and a 4096 x 14336 FFN up-projection, and a 128-row prefill
    for (kq, nq, rows_list) in ((4096, 4096, (1, 128)), (4096, 14336, (1,))):
        bsq = 32
        wq, wsc = dev(rng.integers(0, 256, (nq, kq // bsq, bsq // 2)).astype(np.uint8)), dev(rng.random((nq, kq // bsq), dtype=np.float32) * 0.01)
        for rows_q in rows_list:
            xq, yq = dev(rng.standard_normal((rows_q, kq), dtype=np.float32)), empty((rows_q, nq))
            fn = (lambda xq=xq, yq=yq, rows_q=rows_q, kq=kq, nq=nq, wq=wq, wsc=wsc: ctx.call("rten_hip_matmul_nbits_f32", 1, rows_q, kq, nq, bsq, xq.vp, wq.vp, wsc.vp, yq.vp))
            if rows_q == 1:
                hbm("MatMulNBits decode", f"1x{kq}x{nq} q4/{bsq}", fn, nq * kq / 2 + 4.0 * (nq * kq // bsq + kq + nq))
            else:
                mfma("MatMulNBits prefill", f"{rows_q}x{kq}x{nq} q4/{bsq}", fn, 2.0 * rows_q * kq * nq, F32_PEAK_TF, "TFLOP/s")

    # ---- ReduceSum through strides and Einsum (src/ops/reduce.rs, src/ops/einsum.rs): a contiguous last-axis sum, a column sum over
    # the strided axis (nothing packed), and the two attention products written as Einsum on un-transposed [B, S, H, D]
    # projections (one strided two-level batched GEMM each; the second also pays the output permutation copy)
    from rten_amd import ops as _ops
    ctx.enable_pool(True)  # operator-level rows: outputs and intermediates come from the buffer pool, as under a graph executor
    xr = dev(rng.standard_normal((32 * 12 * 128, 128), dtype=np.float32))
    rs_last, rs_first = _ops.ReduceSum(axes=[1], keep_dims=False), _ops.ReduceSum(axes=[0], keep_dims=False)

    def graphed(fn):  # run once (fills the pool), capture one evaluation into a hipGraph, time replays of it
        fn()  # results return to the pool at once, so the captured evaluation allocates nothing
        fn()
        ctx.sync()
        ctx.graph_begin()
        keep = fn()  # held by the closure: the graph's output buffer is not handed out again while it is replayed
        g = ctx.graph_end()
        return lambda keep=keep: ctx.graph_launch(g)
    # (these two straight through the C entry, like the other single-kernel rows: the replay of a ONE-kernel hipGraph has a ~9.6 us floor of its
    # own, which is what rounds 2-3 reported for the last-axis sum whatever its kernel did)
    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    yr = empty((49152,))
    hbm("ReduceSum last axis", "49152x128", (lambda: ctx.call("rten_hip_reduce_sum_strided_f32", 1, i64(49152), i64(128), 1, i64(128), i64(1), xr.vp, yr.vp)),
        4.0 * (49152 * 128 + 49152))
    xc = dev(rng.standard_normal((4096, 3072), dtype=np.float32))
    yc = empty((3072,))
    hbm("ReduceSum strided axis", "4096x3072 -> 3072", (lambda: ctx.call("rten_hip_reduce_sum_strided_f32", 1, i64(3072), i64(1), 1, i64(4096), i64(3072), xc.vp, yc.vp)),
        4.0 * (4096 * 3072 + 3072))
    # ---- the selection family (rten_amd/csrc/select.hip): ReduceMax on the two ReduceSum shapes above (its yardstick is the ReduceSum row of the same run),
    # ArgMax over the channels of a segmentation map and over logits rows, a whole-tensor ReduceMax (yardstick: a device copy of the input's size), TopK.
    # bytes = input once + output once.
    hbm("ReduceMax last axis", "49152x128", (lambda: ctx.call("rten_hip_reduce_minmax_strided", 0, 0, 1, i64(49152), i64(128), 1, i64(128), i64(1), xr.vp, yr.vp)),
        4.0 * (49152 * 128 + 49152))
    hbm("ReduceMax strided axis", "4096x3072 -> 3072", (lambda: ctx.call("rten_hip_reduce_minmax_strided", 0, 0, 1, i64(3072), i64(1), 1, i64(4096), i64(3072), xc.vp, yc.vp)),
        4.0 * (4096 * 3072 + 3072))
    # ---- the rest of the Reduce* family and LpNormalization (rten_amd/csrc/reduce.hip) on the two ReduceSum shapes above.  L1 / SumSquare / L2 move
    # ReduceSum's bytes through ReduceSum's kernels, so their yardstick is ReduceSum ITSELF, timed in the same loop: the rows of a shape are timed one
    # after the other, `rounds` times over, and every row reports the median with the fastest and slowest round (the run-to-run spread the comparison
    # has to be read against).  LogSumExp and LpNormalization are reported as bytes/s against the HBM peak: one-read forms at these sizes.
    def alternating(group, specs, rounds=5):
        specs = [s for s in specs if want(s[0])]
        if not specs:
            return
        samples = {s[0]: [] for s in specs}
        for _ in range(rounds):
            for op, shape, fn, nbytes in specs:
                samples[op].append(timeit(fn))
        for op, shape, fn, nbytes in specs:
            t = sorted(samples[op])
            us = t[len(t) // 2]
            gbs = nbytes / us / 1e3
            rows.append({"op": op, "shape": shape, "us": round(us, 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2), "rounds": rounds, "group": group, "bound": "hbm",
                         "achieved": round(gbs, 1), "unit": "GB/s", "peak": HBM_PEAK_GBS, "frac": round(gbs / HBM_PEAK_GBS, 3), "algorithmic_bytes": int(nbytes)})

    def red(kind, dt=0):
        last = (lambda: ctx.call("rten_hip_reduce_strided", kind, dt, 1, i64(49152), i64(128), 1, i64(128), i64(1), xr.vp, yr.vp))
        cols = (lambda: ctx.call("rten_hip_reduce_strided", kind, dt, 1, i64(3072), i64(1), 1, i64(4096), i64(3072), xc.vp, yc.vp))
        return last, cols
    b_last, b_cols = 4.0 * (49152 * 128 + 49152), 4.0 * (4096 * 3072 + 3072)
    sum_last = (lambda: ctx.call("rten_hip_reduce_sum_strided_f32", 1, i64(49152), i64(128), 1, i64(128), i64(1), xr.vp, yr.vp))
    sum_cols = (lambda: ctx.call("rten_hip_reduce_sum_strided_f32", 1, i64(3072), i64(1), 1, i64(4096), i64(3072), xc.vp, yc.vp))
    alternating("reduce last axis", [("reduce: ReduceSum last axis (yardstick)", "49152x128", sum_last, b_last),
                                     ("reduce: ReduceL1 last axis", "49152x128", red(0)[0], b_last),
                                     ("reduce: ReduceSumSquare last axis", "49152x128", red(1)[0], b_last),
                                     ("reduce: ReduceL2 last axis", "49152x128", red(2)[0], b_last),
                                     ("reduce: ReduceLogSumExp last axis (one read)", "49152x128", red(4)[0], b_last),
                                     ("reduce: ReduceProd last axis", "49152x128", red(5)[0], b_last)])
    alternating("reduce strided axis", [("reduce: ReduceSum strided axis (yardstick)", "4096x3072 -> 3072", sum_cols, b_cols),
                                        ("reduce: ReduceL1 strided axis", "4096x3072 -> 3072", red(0)[1], b_cols),
                                        ("reduce: ReduceSumSquare strided axis", "4096x3072 -> 3072", red(1)[1], b_cols),
                                        ("reduce: ReduceL2 strided axis", "4096x3072 -> 3072", red(2)[1], b_cols),
                                        ("reduce: ReduceLogSumExp strided axis (two reads)", "4096x3072 -> 3072", red(4)[1], 2 * b_cols)])
    lp_specs = []
    for rows_lp in (16384, 32):
        xl_ = dev(rng.standard_normal((rows_lp, 768), dtype=np.float32))
        yl_ = empty((rows_lp, 768))
        lp_specs.append(("reduce: LpNormalization p=2 (one read, one write)", f"{rows_lp}x768",
                         (lambda xl_=xl_, yl_=yl_, rows_lp=rows_lp: ctx.call("rten_hip_lp_normalize_f32", 2, 1, i64(rows_lp), i64(768), 768, 1, xl_.vp, yl_.vp)), 8.0 * rows_lp * 768))
        lp_specs.append(("reduce: copy, LpNormalization's size (reference point)", f"{rows_lp}x768",
                         (lambda xl_=xl_, yl_=yl_, rows_lp=rows_lp: ctx.call("rten_hip_memcpy_d2d", yl_.vp, xl_.vp, C.c_size_t(4 * rows_lp * 768))), 8.0 * rows_lp * 768))
    for k in range(0, len(lp_specs), 2):  # (two specs share a name across the shapes: one group per shape keeps their samples apart)
        alternating("LpNormalization " + lp_specs[k][1], lp_specs[k:k + 2])
    # ---- GridSample (rten_amd/csrc/sample.hip) and DepthToSpace (one rten_hip_transpose_b32 launch on a 6-D view).  Bytes: x and y once, the grid's
    # 8 bytes per output pixel.  The identity-grid row reads what a same-size bilinear Resize reads and writes the same output, so that Resize
    # (existing code) is timed beside it in the same loop, round by round; a uniformly random grid is the gather's worst case.
    from rten_amd import onnx_writer as _ow

    def gs_rows(label, n_, c_, h_, w_, oh_, ow_, grid_np, with_resize=False):
        xg_ = dev(rng.standard_normal((n_, c_, h_, w_), dtype=np.float32))
        gg_, yg_ = dev(grid_np), empty((n_, c_, oh_, ow_))
        nbytes = 4.0 * n_ * c_ * (h_ * w_ + oh_ * ow_)
        gbytes = 8.0 * n_ * oh_ * ow_
        shape = f"{n_}x{c_}x{h_}x{w_} at {n_}x{oh_}x{ow_}x2"
        specs = [(f"image: GridSample {label}", shape, (lambda: ctx.call("rten_hip_grid_sample_f32", 0, n_, c_, h_, w_, oh_, ow_, xg_.vp, gg_.vp, yg_.vp)), nbytes + gbytes)]
        if with_resize:
            specs.append(("image: Resize linear half_pixel, same input and output size (yardstick)", f"{n_}x{c_}x{h_}x{w_} -> {oh_}x{ow_}",
                          (lambda: ctx.call("rten_hip_resize_f32", L.RESIZE_MODE_LINEAR, L.RESIZE_COORD_HALF_PIXEL, L.RESIZE_NEAREST_FLOOR, n_ * c_, h_, w_, oh_, ow_,
                                            h_ / oh_, w_ / ow_, xg_.vp, yg_.vp)), nbytes))
        before = len(rows)
        alternating(f"GridSample {label} {shape}", specs)
        for row in rows[before:]:
            if row["op"].startswith("image: GridSample"):
                row["grid_bytes"] = int(gbytes)
    if want("image: GridSample"):
        ident = lambda n_, h_, w_: np.ascontiguousarray(np.broadcast_to(_ow.base_grid(h_, w_), (n_, h_, w_, 2)))
        gs_rows("identity grid", 8, 64, 128, 128, 128, 128, ident(8, 128, 128), with_resize=True)
        gs_rows("random grid", 8, 64, 128, 128, 128, 128, rng.uniform(-1, 1, (8, 128, 128, 2)).astype(np.float32))
        gs_rows("flow warp (identity + N(0, 0.05))", 2, 3, 512, 512, 512, 512, (ident(2, 512, 512) + rng.normal(0, 0.05, (2, 512, 512, 2))).astype(np.float32))
        gs_rows("deformable attention points", 64, 32, 32, 32, 100, 4, rng.uniform(-1, 1, (64, 100, 4, 2)).astype(np.float32))
    if want("image: DepthToSpace"):
        nd2s = 8 * 256 * 128 * 128
        xd_, yd_ = dev(rng.standard_normal((nd2s,), dtype=np.float32)), empty((nd2s,))
        i32 = lambda *v: (C.c_int32 * len(v))(*v)
        alternating("DepthToSpace 8x256x128x128", [
            ("image: DepthToSpace DCR block 2 (one 6-D transpose)", "8x256x128x128 -> 8x64x256x256",
             (lambda: ctx.call("rten_hip_transpose_b32", 6, i64(8, 2, 2, 64, 128, 128), i32(0, 3, 4, 1, 5, 2), xd_.vp, yd_.vp)), 8.0 * nd2s),
            ("image: DepthToSpace CRD block 2 (one 6-D transpose)", "8x256x128x128 -> 8x64x256x256",
             (lambda: ctx.call("rten_hip_transpose_b32", 6, i64(8, 64, 2, 2, 128, 128), i32(0, 1, 4, 2, 5, 3), xd_.vp, yd_.vp)), 8.0 * nd2s),
            ("image: copy, DepthToSpace's size (reference point)", f"{4 * nd2s} B", (lambda: ctx.call("rten_hip_memcpy_d2d", yd_.vp, xd_.vp, C.c_size_t(4 * nd2s))), 8.0 * nd2s)])
        del xd_, yd_
    # ---- CumSum / GatherElements / Trilu / Tile (rten_amd/csrc/scan.hip).  CumSum beside ReduceSum on the same shape (existing code; CumSum also WRITES the
    # tensor, so its bytes are twice ReduceSum's), the other three beside a rten_hip_copy_strided_b32 of the same output (8 bytes per element; GatherElements
    # also reads 4 bytes of index per element).  Each group is timed round by round in one loop.
    if want("index:"):
        ycs, ycc = empty((49152, 128)), empty((4096, 3072))
        xri, xci = dev(rng.integers(-1000, 1000, (49152, 128)).astype(np.int32)), dev(rng.integers(-1000, 1000, (4096, 3072)).astype(np.int32))
        cs = lambda dt, outer, n, inner, src, dst: (lambda: ctx.call("rten_hip_cumsum_b32", dt, 0, 0, outer, n, inner, src.vp, dst.vp))
        alternating("CumSum last axis 49152x128", [
            ("index: CumSum f32 last axis (row form)", "49152x128", cs(0, 49152, 128, 1, xr, ycs), 8.0 * 49152 * 128),
            ("index: CumSum int32 last axis (row form)", "49152x128", cs(1, 49152, 128, 1, xri, ycs), 8.0 * 49152 * 128),
            ("index: ReduceSum last axis (yardstick)", "49152x128", sum_last, b_last)])
        alternating("CumSum axis 0 4096x3072", [
            ("index: CumSum f32 axis 0 (column form)", "4096x3072", cs(0, 1, 4096, 3072, xc, ycc), 8.0 * 4096 * 3072),
            ("index: CumSum int32 axis 0 (column form)", "4096x3072", cs(1, 1, 4096, 3072, xci, ycc), 8.0 * 4096 * 3072),
            ("index: ReduceSum strided axis (yardstick)", "4096x3072 -> 3072", sum_cols, b_cols)])
        sum_rows = (lambda: ctx.call("rten_hip_reduce_sum_strided_f32", 1, i64(4096), i64(3072), 1, i64(3072), i64(1), xc.vp, yr.vp))
        alternating("CumSum last axis 4096x3072", [
            ("index: CumSum f32 last axis of long rows (row form)", "4096x3072", cs(0, 4096, 3072, 1, xc, ycc), 8.0 * 4096 * 3072),
            ("index: ReduceSum last axis of long rows (yardstick)", "4096x3072 -> 4096", sum_rows, 4.0 * (4096 * 3072 + 4096))])
        one_lane = (lambda: ctx.call("rten_hip_reduce_sum_strided_f32", 1, i64(1), i64(1), 1, i64(1 << 20), i64(1), xc.vp, yc.vp))
        alternating("CumSum single lane", [
            ("index: CumSum f32 ONE lane of 2^20 (serial by contract)", "1x1048576", cs(0, 1, 1 << 20, 1, xc, ycc), 8.0 * (1 << 20)),
            ("index: ReduceSum of the same lane (yardstick)", "1x1048576 -> 1", one_lane, 4.0 * (1 << 20))])
        alternating("CumSum position ids 32x512", [
            ("index: CumSum int32 position ids (row form)", "32x512", cs(1, 32, 512, 1, xri, ycs), 8.0 * 32 * 512),
            ("index: ReduceSum of the same rows (yardstick)", "32x512 -> 32", (lambda: ctx.call("rten_hip_reduce_sum_strided_f32", 1, i64(32), i64(512), 1, i64(512), i64(1), xr.vp, yr.vp)),
             4.0 * (32 * 512 + 32))])
        n_ge = 4096 * 3072
        copy2d = (lambda: ctx.call("rten_hip_copy_strided_b32", 2, i64(4096, 3072), i64(3072, 1), xc.vp, ycc.vp))
        ids_in = dev(rng.integers(0, 3072, (4096, 3072)).astype(np.int32))
        ids_out = dev(rng.integers(0, 4096, (4096, 3072)).astype(np.int32))
        alternating("GatherElements 4096x3072", [
            ("index: GatherElements innermost axis, random indices", "4096x3072", (lambda: ctx.call("rten_hip_gather_elements_b32", 2, i64(4096, 3072), i64(4096, 3072), 1, xc.vp, ids_in.vp, ycc.vp)), 12.0 * n_ge),
            ("index: GatherElements axis 0, random indices (a row per element)", "4096x3072", (lambda: ctx.call("rten_hip_gather_elements_b32", 2, i64(4096, 3072), i64(4096, 3072), 0, xc.vp, ids_out.vp, ycc.vp)), 12.0 * n_ge),
            ("index: strided copy of the same tensor (yardstick)", "4096x3072", copy2d, 8.0 * n_ge)])
        del ids_in, ids_out
        alternating("Trilu 48x512x512", [
            ("index: Trilu upper, k = 1", "48x512x512", (lambda: ctx.call("rten_hip_trilu_b32", 1, 1, 48, 512, 512, xc.vp, ycc.vp)), 8.0 * n_ge),
            ("index: strided copy of the same tensor (yardstick)", "48x512x512", (lambda: ctx.call("rten_hip_copy_strided_b32", 3, i64(48, 512, 512), i64(512 * 512, 512, 1), xc.vp, ycc.vp)), 8.0 * n_ge)])
        alternating("Tile 512x768 x (8, 3)", [
            ("index: Tile rows and columns", "512x768 x (8, 3) -> 4096x2304", (lambda: ctx.call("rten_hip_tile_b32", 2, i64(512, 768), i64(8, 3), xc.vp, ycc.vp)), 4.0 * (4096 * 2304 + 512 * 768)),
            ("index: Tile as Tensor.repeat(1, 3, 2) of a decoder output", "64x1x768 x (1, 3, 2)", (lambda: ctx.call("rten_hip_tile_b32", 3, i64(64, 1, 768), i64(1, 3, 2), xc.vp, ycc.vp)), 4.0 * 64 * 768 * 7),
            ("index: broadcasting strided copy to the same output (yardstick)", "-> 4096x2304", (lambda: ctx.call("rten_hip_copy_strided_b32", 2, i64(4096, 2304), i64(2304, 1), xc.vp, ycc.vp)), 8.0 * 4096 * 2304)])
        del ycs, ycc, xri, xci
    # ---- NonMaxSuppression (rten_amd/csrc/nms.hip) on a detector's post-processing shape: 8400 boxes x 80 classes, one image and 32, at a score threshold that
    # leaves about 100 candidates per image and at one that leaves all of them.  The call synchronises (it reads the row count back), so a row is the host's
    # wall time around ONE call, median of `rounds` after a warm-up call; beside it the per-kernel times of the same call from the launch profiler -- the
    # class walk (step 1, HBM-bound: it reads every score once; its yardstick is the existing ReduceMax over the class axis of the same scores, timed the usual
    # way), the serial resolve on its own, and the sort / cap / rows launch.  The resolve is ONE workgroup and serial by contract: latency-bound, one barrier
    # and a dependent load chain per candidate, plus the iou of the candidate against every member alive at that point.
    if want("nms:"):
        import time

        def nms_rows(images, per_image, rounds=5):
            nb_, nc_ = 8400, 80
            cx, cy = rng.uniform(0, 640, (images, nb_)), rng.uniform(0, 640, (images, nb_))
            w_, h_ = rng.uniform(20, 200, (images, nb_)), rng.uniform(20, 200, (images, nb_))
            bx = dev(np.stack([cx, cy, w_, h_], axis=-1).astype(np.float32))
            sc_np = (rng.random((images, nc_, nb_)) ** 8).astype(np.float32)
            best = np.sort(sc_np.max(axis=1).reshape(-1))
            thr = float(best[-per_image * images]) if per_image < nb_ else -1.0
            sc, out_rows, ymax = dev(sc_np), empty((images * nb_, 3), np.int32), empty((images, nb_))
            count = C.c_int64(0)
            call = (lambda: ctx.call("rten_hip_non_max_suppression_f32", 1, images, nc_, nb_, bx.vp, sc.vp, 0, 0, C.c_float(0.5), C.c_float(thr), out_rows.vp, C.byref(count)))
            call()
            wall, kernels = [], {}
            for _ in range(rounds):
                ctx.profile_reset()
                ctx.profile(True)
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e6)
                ctx.profile(False)
                for e in ctx.profile_report():
                    if str(e.get("kernel", "")).startswith("nms_"):
                        kernels.setdefault(e["kernel"], []).append(float(e.get("ms", 0.0)) * 1e3)
            wall.sort()
            shape = f"{images}x{nb_} boxes x {nc_} classes, {per_image if per_image < nb_ else nb_} candidates per image, iou 0.5 -> {count.value} rows"
            nbytes = 4.0 * images * nb_ * (nc_ + 4)
            rows.append({"op": "nms: NonMaxSuppression, whole call (host wall time, one sync)", "shape": shape, "us": round(wall[len(wall) // 2], 2), "us_min": round(wall[0], 2),
                         "us_max": round(wall[-1], 2), "rounds": rounds, "group": "nms", "bound": "latency (one workgroup, serial by contract)", "algorithmic_bytes": int(nbytes),
                         "rows": int(count.value)})
            for name, bound in (("nms_class_f32", "hbm"), ("nms_offsets", "latency"), ("nms_gather_f32", "hbm"), ("nms_resolve", "latency (one workgroup, serial by contract)"),
                                ("nms_order", "latency (one workgroup)")):
                t = sorted(kernels.get(name, [0.0]))
                row = {"op": f"nms: {name} (launch profiler)", "shape": shape, "us": round(t[len(t) // 2], 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2), "rounds": rounds,
                       "group": "nms", "bound": bound}
                if name == "nms_class_f32" and row["us"] > 0:
                    gbs = 4.0 * images * nb_ * nc_ / row["us"] / 1e3
                    row.update({"achieved": round(gbs, 1), "unit": "GB/s", "peak": HBM_PEAK_GBS, "frac": round(gbs / HBM_PEAK_GBS, 3), "algorithmic_bytes": int(4.0 * images * nb_ * nc_)})
                rows.append(row)
            alternating(f"nms class walk {images}x{nc_}x{nb_}", [
                ("nms: ReduceMax over the class axis of the same scores (yardstick for nms_class_f32)", f"{images}x{nc_}x{nb_} -> {images}x{nb_}",
                 (lambda: ctx.call("rten_hip_reduce_minmax_strided", 0, 0, 2, i64(images, nb_), i64(nc_ * nb_, 1), 1, i64(nc_), i64(nb_), sc.vp, ymax.vp)), 4.0 * images * nb_ * (nc_ + 1))])

        nms_rows(1, 100)
        nms_rows(1, 8400)
        nms_rows(32, 100)
        nms_rows(32, 8400, rounds=3)
    xs = dev(rng.standard_normal((1, 21, 512, 512), dtype=np.float32))
    ys = empty((512 * 512,), np.int32)
    hbm("ArgMax over channels", "1x21x512x512", (lambda: ctx.call("rten_hip_arg_minmax_strided", 0, 0, 1, i64(512 * 512), i64(1), 21, 512 * 512, xs.vp, ys.vp)),
        4.0 * (21 * 512 * 512 + 512 * 512))
    hbm("copy, ArgMax over channels' size (reference point)", f"{4 * 21 * 512 * 512} B",
        (lambda: ctx.call("rten_hip_memcpy_d2d", xc.vp, xs.vp, C.c_size_t(4 * 21 * 512 * 512))), 8.0 * 21 * 512 * 512)
    xl = dev(rng.standard_normal((32, 1000), dtype=np.float32))
    yl = empty((32,), np.int32)
    hbm("ArgMax last axis", "32x1000", (lambda: ctx.call("rten_hip_arg_minmax_strided", 0, 0, 1, i64(32), i64(1000), 1000, 1, xl.vp, yl.vp)), 4.0 * (32 * 1000 + 32))
    hbm("copy, ArgMax last axis' size (reference point)", f"{4 * 32 * 1000} B", (lambda: ctx.call("rten_hip_memcpy_d2d", xc.vp, xl.vp, C.c_size_t(4 * 32 * 1000))), 8.0 * 32 * 1000)
    nw = 32 * 64 * 112 * 112
    xw = dev(rng.standard_normal((nw,), dtype=np.float32))
    xw2 = empty((nw,))
    hbm("ReduceMax whole tensor", "32x64x112x112", (lambda: ctx.call("rten_hip_reduce_minmax_strided", 0, 0, 0, i64(), i64(), 1, i64(nw), i64(1), xw.vp, yl.vp)), 4.0 * (nw + 1))
    hbm("copy, ReduceMax whole tensor's size (reference point)", f"{4 * nw} B", (lambda: ctx.call("rten_hip_memcpy_d2d", xw2.vp, xw.vp, C.c_size_t(4 * nw))), 8.0 * nw)
    for (lanes_t, len_t, k_t, shape_t) in ((32, 1000, 5, "32x1000, k=5"), (8, 8400, 300, "8x8400, k=300"), (1, 151936, 50, "1x151936, k=50"), (32 * 128, 128, 8, "32x128x128, k=8")):
        xt = dev(rng.standard_normal((lanes_t, len_t), dtype=np.float32))
        vt, it = empty((lanes_t, k_t)), empty((lanes_t, k_t), np.int32)
        hbm("TopK", shape_t, (lambda xt=xt, vt=vt, it=it, lanes_t=lanes_t, len_t=len_t, k_t=k_t: ctx.call(
            "rten_hip_topk_strided", 1, 0, 1, i64(lanes_t), i64(len_t), i64(k_t), len_t, 1, k_t, xt.vp, vt.vp, it.vp, 1)), 4.0 * lanes_t * len_t)
    Be, Se, He, De = 32, 128, 12, 64
    qe, ke, ve = (dev(rng.standard_normal((Be, Se, He, De), dtype=np.float32)) for _ in range(3))
    pe = dev(rng.standard_normal((Be, He, Se, Se), dtype=np.float32))
    es, ec = _ops.Einsum("bqhd,bkhd->bhqk"), _ops.Einsum("bhqk,bkhd->bqhd")
    mfma("Einsum bqhd,bkhd->bhqk", f"{Be}x{Se}x{He}x{De}", graphed(lambda: es.run(ctx, [qe, ke])), 2.0 * Be * He * Se * Se * De, F32_PEAK_TF, "TFLOP/s")
    mfma("Einsum bhqk,bkhd->bqhd", f"{Be}x{He}x{Se}x{Se}", graphed(lambda: ec.run(ctx, [pe, ve])), 2.0 * Be * He * Se * Se * De, F32_PEAK_TF, "TFLOP/s")
    ctx.enable_pool(False)

    # ---- f32 GEMM on BERT-base shapes (batch 32 x 128 tokens)
    for (m, k, n, act, name) in ((4096, 768, 768, 0, "MatMul proj"), (4096, 768, 3072, L.ACT_GELU, "MatMul FFN1 + Gelu"), (4096, 3072, 768, 0, "MatMul FFN2")):
        a, w, bias, out = dev(rng.standard_normal((m, k), dtype=np.float32)), dev(rng.standard_normal((k, n), dtype=np.float32)), dev(np.zeros(n, np.float32)), empty((m, n))
        d = L.gemm_desc(m, n, k, k, 1, n, 1, n, bias_kind=L.BIAS_PER_COL, act=act)
        mfma(name, f"{m}x{k}x{n}", (lambda: ctx.call("rten_hip_gemm_f32", C.byref(d), a.vp, w.vp, bias.vp, out.vp)), 2.0 * m * k * n, F32_PEAK_TF, "TFLOP/s")
    # ---- few rows against a big weight matrix (ResNet-50's classifier, Gemm transB = 1; an LLM-decoder projection at 16 rows): bound by streaming B
    for (m, k, n, trans_b, name) in ((32, 2048, 1000, True, "Gemm classifier"), (16, 4096, 4096, False, "MatMul 16 rows")):
        a, w, bias, out = dev(rng.standard_normal((m, k), dtype=np.float32)), dev(rng.standard_normal((n, k) if trans_b else (k, n), dtype=np.float32)), dev(np.zeros(n, np.float32)), empty((m, n))
        d = L.gemm_desc(m, n, k, k, 1, 1 if trans_b else n, k if trans_b else 1, n, bias_kind=L.BIAS_PER_COL)
        hbm(name, f"{m}x{k}x{n}", (lambda: ctx.call("rten_hip_gemm_f32", C.byref(d), a.vp, w.vp, bias.vp, out.vp)), 4.0 * (m * k + k * n + m * n + n))
        ctx.set_gemm_variant(3)
        hbm(name + " (64x64 tiles, round 4)", f"{m}x{k}x{n}", (lambda: ctx.call("rten_hip_gemm_f32", C.byref(d), a.vp, w.vp, bias.vp, out.vp)), 4.0 * (m * k + k * n + m * n + n))
        ctx.set_gemm_variant(-1)
    # attention core, 12 heads x 64 on [B, S, H*D] projections (strided heads)
    B, S, H, D = 32, 128, 12, 64
    q, kk, v, o = (dev(rng.standard_normal((B, S, H * D), dtype=np.float32)) for _ in range(4))
    sd = L.SdpaDesc(B, H, S, S, D, D, S * H * D, D, H * D, S * H * D, D, H * D, S * H * D, D, H * D, S * H * D, D, H * D, 0, 0, 0.125, 0)
    mfma("sdpa (QK^T, softmax, PV)", f"b={B} h={H} s={S} d={D}", (lambda: ctx.call("rten_hip_sdpa_f32", C.byref(sd), q.vp, kk.vp, v.vp, None, o.vp)),
         4.0 * B * H * S * S * D, F32_PEAK_TF, "TFLOP/s")

    # the general one-kernel form (round 3): head 128 x 512 keys (2 query tiles per head), head 64 x 384 keys, head 32 x 256 keys
    for (B2, H2, S2, T2, D2) in ((8, 16, 256, 512, 128), (16, 12, 384, 384, 64), (32, 8, 256, 256, 32), (16, 12, 256, 256, 64), (8, 16, 256, 256, 128), (32, 8, 128, 128, 128),
                                 (32, 16, 128, 128, 32), (16, 12, 256, 200, 64)):
        q2, o2 = dev(rng.standard_normal((B2, H2, S2, D2), dtype=np.float32)), empty((B2, H2, S2, D2))
        k2, v2 = dev(rng.standard_normal((B2, H2, T2, D2), dtype=np.float32)), dev(rng.standard_normal((B2, H2, T2, D2), dtype=np.float32))
        sd2 = L.SdpaDesc(B2, H2, S2, T2, D2, D2, H2 * S2 * D2, S2 * D2, D2, H2 * T2 * D2, T2 * D2, D2, H2 * T2 * D2, T2 * D2, D2, H2 * S2 * D2, S2 * D2, D2, 0, 0,
                         float(1.0 / np.sqrt(D2)), 0)
        for path, label in ((2, "one kernel"), (1, "composed: GEMM, softmax, GEMM")):
            def fn(sd2=sd2, q2=q2, k2=k2, v2=v2, o2=o2):
                ctx.call("rten_hip_sdpa_f32", C.byref(sd2), q2.vp, k2.vp, v2.vp, None, o2.vp)
            ctx.call("rten_hip_set_sdpa_path", path)
            mfma(f"sdpa general ({label})", f"b={B2} h={H2} s={S2} t={T2} d={D2}", fn, 4.0 * B2 * H2 * S2 * T2 * D2, F32_PEAK_TF, "TFLOP/s")
            ctx.call("rten_hip_set_sdpa_path", 0)

    # ---- recurrent layers at a text-recogniser size (bidirectional, 128 columns, 256 features, hidden 256), batch 32 and batch 1: the time-persistent
    #      fused kernel against per-step launches (f32 GEMM + gate kernel).  Each row also carries us per time step.
    for lstm in (False, True):
        for batch in (32, 1):
            seq, n_in, hid, G = 128, 256, 256, 4 if lstm else 3
            xr = dev(rng.standard_normal((seq, batch, n_in), dtype=np.float32))
            wr = dev(rng.standard_normal((2, G * hid, n_in), dtype=np.float32) / 16)
            rr = dev(rng.standard_normal((2, G * hid, hid), dtype=np.float32) / 16)
            br = dev(rng.standard_normal((2, 2 * G * hid), dtype=np.float32) / 4)
            yr, yh, yc = empty((seq, 2, batch, hid)), empty((2, batch, hid)), empty((2, batch, hid))
            geo = (seq, batch, n_in, hid, L.RNN_BIDIRECTIONAL)
            for path, label in ((L.RNN_PATH_FUSED, "fused: one launch walks all steps"), (L.RNN_PATH_COMPOSED, "composed: GEMM + gate kernel per step")):
                def fn(lstm=lstm, geo=geo, xr=xr, wr=wr, rr=rr, br=br, yr=yr, yh=yh, yc=yc):
                    if lstm:
                        ctx.call("rten_hip_lstm_f32", *geo, 0, 0, xr.vp, wr.vp, rr.vp, br.vp, None, None, yr.vp, yh.vp, yc.vp)
                    else:
                        ctx.call("rten_hip_gru_f32", *geo, 1, 0, 0, xr.vp, wr.vp, rr.vp, br.vp, None, yr.vp, yh.vp)
                ctx.call("rten_hip_set_rnn_path", path)
                before = len(rows)
                mfma(f"{'LSTM' if lstm else 'GRU'} bidirectional ({label})", f"seq={seq} batch={batch} input={n_in} hidden={hid}", fn,
                     2.0 * 2 * seq * batch * G * hid * (n_in + hid), F32_PEAK_TF, "TFLOP/s")
                ctx.call("rten_hip_set_rnn_path", L.RNN_PATH_AUTO)
                for row in rows[before:]:
                    row["us_per_step"] = round(row["us"] / seq, 2)

    # ---- int8 GEMM / conv (u8 activations x i8 weights)
    for (m, k, n) in ((4096, 768, 768), (4096, 768, 3072)):
        a = dev(rng.integers(0, 255, (m, k)).astype(np.uint8)); w = dev(rng.integers(-127, 127, (k, n)).astype(np.int8))
        az, wz, out = dev(np.array(128, np.uint8)), dev(np.zeros(n, np.int8)), empty((m, n), np.int32)
        d = L.GemmInt8Desc(m, n, k, k, 1, n, 1, n, 0, 1, 1, n, 0)
        mfma("MatMulInteger", f"{m}x{k}x{n}", (lambda: ctx.call("rten_hip_gemm_int8", C.byref(d), a.vp, w.vp, az.vp, wz.vp, None, out.vp)), 2.0 * m * k * n, I8_PEAK_TOPS, "TOP/s")
        nb = ctx.lib.rten_hip_gemm_int8_packed_bytes(k, n)  # constant RHS staged once at load (Operator::prepack): the per-call staging of B disappears
        if nb:
            packed = empty((nb,), np.uint8)
            ctx.call("rten_hip_gemm_int8_prepack", k, n, w.vp, n, 1, 1, packed.vp)
            dp = L.GemmInt8Desc(m, n, k, k, 1, n, 1, n, 0, 1, 1, n, 0, 1, 0, 0, 0, 1)
            mfma("MatMulInteger (prepacked RHS)", f"{m}x{k}x{n}", (lambda: ctx.call("rten_hip_gemm_int8", C.byref(dp), a.vp, packed.vp, az.vp, wz.vp, None, out.vp)),
                 2.0 * m * k * n, I8_PEAK_TOPS, "TOP/s")
    for (o_, c_, hw, k_, s_, p_, name) in ((64, 64, 56, 3, 1, 1, "s0 3x3"), (256, 256, 14, 3, 1, 1, "s2 3x3"), (256, 64, 56, 1, 1, 0, "s0 1x1 expand")):
        xq = dev(rng.integers(0, 255, (32, c_, hw, hw)).astype(np.uint8)); wq = dev(rng.integers(-127, 127, (o_, c_, k_, k_)).astype(np.int8))
        xz, wz = dev(np.array(128, np.uint8)), dev(np.zeros(o_, np.int8))
        oh = (hw + 2 * p_ - k_) // s_ + 1
        out = empty((32, o_, oh, oh), np.int32)
        cd = L.Conv2dDesc(32, c_, hw, hw, o_, k_, k_, (C.c_int32 * 4)(p_, p_, p_, p_), s_, s_, 1, 1, 1, oh, oh)
        d = L.Conv2dInt8Desc(cd, 0, 1, o_, 1)
        mfma(f"ConvInteger {name}", f"32x{c_}x{hw}x{hw} -> {o_}, k{k_}",
             (lambda: ctx.call("rten_hip_conv2d_int8", C.byref(d), xq.vp, wq.vp, xz.vp, wz.vp, None, None, None, 0, out.vp)),
             2.0 * 32 * o_ * c_ * k_ * k_ * oh * oh, I8_PEAK_TOPS, "TOP/s")

    # ---- DFT / STFT (rten_amd/csrc/fft.hip): one LDS-resident Stockham FFT per lane; a call is the twiddle prologue plus one transform launch.  The HBM bound
    # is for the bytes the call must move: the signal once, the output once (overlapping STFT frames re-read the signal from cache, not from HBM).
    if want("fft:"):
        for b_ in (1, 8):
            sig, win = dev(rng.standard_normal((b_, 480000), dtype=np.float32)), dev(np.hanning(401)[:400].astype(np.float32))
            frames = (480000 - 400) // 160 + 1
            spec = empty((b_, frames, 201, 2))
            hbm("fft: STFT 30 s of 16 kHz audio, n_fft 400, hop 160, Hann window, onesided", f"{b_}x480000 -> {b_}x{frames}x201x2",
                (lambda: ctx.call("rten_hip_stft_f32", b_, 480000, 1, 160, 400, 1, win.vp, sig.vp, spec.vp)), 4.0 * b_ * (480000 + frames * 201 * 2))
            del sig, spec
        xc_, yc_ = dev(rng.standard_normal((4096, 1024, 2), dtype=np.float32)), empty((4096, 1024, 2))
        for inv in (0, 1):
            hbm(f"fft: DFT complex {'inverse' if inv else 'forward'}", "4096 lanes x 1024", (lambda: ctx.call("rten_hip_dft_f32", 4096, 1024, 1024, 2, inv, 0, xc_.vp, yc_.vp)),
                4.0 * 4096 * 1024 * 4)
        xr_, yr_ = dev(rng.standard_normal((4096, 400, 1), dtype=np.float32)), empty((4096, 201, 2))
        hbm("fft: RFFT (real input, onesided)", "4096 lanes x 400 -> 201 bins", (lambda: ctx.call("rten_hip_dft_f32", 4096, 400, 400, 1, 0, 1, xr_.vp, yr_.vp)), 4.0 * 4096 * (400 + 201 * 2))
        hbm("fft: strided copy of the DFT's bytes (yardstick)", "4096x2048", (lambda: ctx.call("rten_hip_copy_strided_b32", 2, (C.c_int64 * 2)(4096, 2048), (C.c_int64 * 2)(2048, 1), xc_.vp, yc_.vp)),
            8.0 * 4096 * 2048)
        del xc_, yc_, xr_, yr_

    # ---- decoder blocks (rten_amd/csrc/decoder.hip): RMS normalisation, the skip form with its sum written, rotary embedding.  Each norm row is followed by
    # the same shape through rten_hip_layer_norm_f32 (up to 1024 columns its register forms, above that its generic one-wave-per-row form: what these rows
    # ran on before) and by a strided copy of the same bytes, the yardstick.  RTEN_NORM_WPR=4 in the environment forces the workgroup-per-row form at 1024
    # columns and below: the two runs side by side are the numbers behind the launch rule's 1024 boundary (docs/KERNELS.md 4.17).
    if want("decoder:"):
        form = os.environ.get("RTEN_NORM_WPR", "rule")
        for r_, c_ in ((1, 4096), (32, 4096), (4096, 4096), (2048, 8192), (32, 1024), (4096, 1024), (4096, 512)):
            xd, sd, yd, td = dev(rng.standard_normal((r_, c_), dtype=np.float32)), dev(rng.standard_normal((r_, c_), dtype=np.float32)), empty((r_, c_)), empty((r_, c_))
            gd, bd = dev(rng.standard_normal(c_, dtype=np.float32)), dev(rng.standard_normal(c_, dtype=np.float32))
            shape = f"rows={r_} cols={c_} form={form}"
            hbm("decoder: RMSNormalization", shape, (lambda: ctx.call("rten_hip_rms_norm_f32", r_, c_, xd.vp, gd.vp, 1.0, 1e-6, yd.vp)), 8.0 * r_ * c_)
            hbm("decoder: LayerNormalization entry point, same shape (what the rows ran on before)", shape,
                (lambda: ctx.call("rten_hip_layer_norm_f32", r_, c_, xd.vp, gd.vp, bd.vp, C.c_float(1.0), C.c_float(0.0), C.c_float(1e-6), yd.vp)), 8.0 * r_ * c_)
            hbm("decoder: strided copy of the norm's bytes (yardstick)", shape,
                (lambda: ctx.call("rten_hip_copy_strided_b32", 2, (C.c_int64 * 2)(r_, c_), (C.c_int64 * 2)(c_, 1), xd.vp, yd.vp)), 8.0 * r_ * c_)
            hbm("decoder: SkipSimplifiedLayerNormalization with the sum written", shape,
                (lambda: ctx.call("rten_hip_skip_norm_f32", 1, r_, c_, xd.vp, sd.vp, r_, None, gd.vp, None, 1e-6, td.vp, yd.vp)), 16.0 * r_ * c_)
            def two_copies():  # the skip form reads two tensors and writes two: the same bytes as two copies, which are two launches
                ctx.call("rten_hip_copy_strided_b32", 2, (C.c_int64 * 2)(r_, c_), (C.c_int64 * 2)(c_, 1), xd.vp, yd.vp)
                ctx.call("rten_hip_copy_strided_b32", 2, (C.c_int64 * 2)(r_, c_), (C.c_int64 * 2)(c_, 1), sd.vp, td.vp)
            hbm("decoder: two strided copies of the skip form's bytes (yardstick)", shape, two_copies, 16.0 * r_ * c_)
            del xd, sd, yd, td
        cos_, sin_ = dev(rng.standard_normal((4096, 64), dtype=np.float32)), dev(rng.standard_normal((4096, 64), dtype=np.float32))
        off_ = dev(np.array([100], np.int32))
        for b_, s_, h_ in ((32, 1, 32), (1, 2048, 32)):
            d_ = 128
            xq, yq = dev(rng.standard_normal((b_, s_, h_ * d_), dtype=np.float32)), empty((b_, s_, h_ * d_))
            shape = f"batch={b_} seq={s_} heads={h_} head_size={d_}"
            hbm("decoder: RotaryEmbedding, positions from a one-element device offset", shape,
                (lambda: ctx.call("rten_hip_rotary_embedding_f32", b_, s_, h_, d_, d_, 0, xq.vp, s_ * h_ * d_, h_ * d_, d_, cos_.vp, 0, 0, sin_.vp, 0, 0, off_.vp, 2, 4096,
                                  yq.vp, s_ * h_ * d_, h_ * d_, d_)), 8.0 * b_ * s_ * h_ * d_)
            hbm("decoder: strided copy of the rotary rows' bytes (yardstick)", shape,
                (lambda: ctx.call("rten_hip_copy_strided_b32", 2, (C.c_int64 * 2)(b_ * s_, h_ * d_), (C.c_int64 * 2)(h_ * d_, 1), xq.vp, yq.vp)), 8.0 * b_ * s_ * h_ * d_)
            del xq, yq

    # ---- GroupQueryAttention with a KV cache (rten_amd/csrc/gqa.hip; --only gqa: selects these rows): decode at H 32 / KV 8 / D 128 on a cache of
    # kv_len - 1 rows, the whole call (prepare-and-append launch + attention) on the decode kernel and on the composed path, beside (a) what such a
    # graph ran on before -- two strided copies for the concatenation, then rten_hip_sdpa_f32 with one query row on K and V expanded to 32 heads -- and
    # (b) one strided copy of the K and V bytes, the yardstick.  Then one first prompt of 2048 tokens.  Operands are zeros: the timing does not read values.
    if want("gqa:"):
        h_, kv_, d_ = 32, 8, 128

        def zeros(*shape, dt=np.float32):
            t_ = empty(shape, dt)
            ctx.call("rten_hip_memset", t_.vp, 0, C.c_size_t(t_.size * 4))
            return t_

        for b_ in (1, 32):
            for kvl in (512, 2048, 4096):
                p_ = kvl - 1
                q_, k_, v_ = zeros(b_, 1, h_ * d_), zeros(b_, 1, kv_ * d_), zeros(b_, 1, kv_ * d_)
                pk_, pv_, ok_, ov_ = zeros(b_, kv_, p_, d_), zeros(b_, kv_, p_, d_), zeros(b_, kv_, kvl, d_), zeros(b_, kv_, kvl, d_)
                o_ = zeros(b_, 1, h_ * d_)
                sl_, tot_ = dev(np.full(b_, kvl - 1, np.int32)), dev(np.array([kvl], np.int32))
                dims = (C.c_int32 * L.GQA_NDIMS)(b_, 1, h_, kv_, d_, p_, 0, 0, 0, 0)
                st_ = (C.c_int64 * L.GQA_NSTRIDES)(h_ * d_, h_ * d_, d_, kv_ * d_, kv_ * d_, d_, kv_ * d_, kv_ * d_, d_, 0, 0, 0)
                shape = f"batch={b_} kv_len={kvl} heads={h_} kv_heads={kv_} head_size={d_}"
                kv_bytes = 8.0 * b_ * kv_ * kvl * d_
                call = (lambda: ctx.call("rten_hip_gqa_f32", dims, st_, 0.0883883461, q_.vp, k_.vp, v_.vp, pk_.vp, pv_.vp, sl_.vp, tot_.vp, None, None, None, None,
                                         o_.vp, ok_.vp, ov_.vp))
                for pname, path in (("decode kernel", 2), ("composed path", 1), ("dispatch rule", 0)):
                    ctx.call("rten_hip_set_gqa_path", path)
                    hbm(f"gqa: decode, whole call ({pname})", shape, call, 3 * kv_bytes)
                ctx.call("rten_hip_set_gqa_path", 0)
                ke_, ve_ = zeros(b_, h_, kvl, d_), zeros(b_, h_, kvl, d_)
                sd_ = L.SdpaDesc(b_, h_, 1, kvl, d_, d_, h_ * d_, d_, h_ * d_, h_ * kvl * d_, kvl * d_, d_, h_ * kvl * d_, kvl * d_, d_, h_ * d_, d_, h_ * d_, 0, 0,
                                 0.0883883461, 1)
                csh, cst = (C.c_int64 * 2)(b_ * kv_ * p_, d_), (C.c_int64 * 2)(d_, 1)

                def parent_route():
                    ctx.call("rten_hip_copy_strided_b32", 2, csh, cst, pk_.vp, ok_.vp)
                    ctx.call("rten_hip_copy_strided_b32", 2, csh, cst, pv_.vp, ov_.vp)
                    ctx.call("rten_hip_sdpa_f32", C.byref(sd_), q_.vp, ke_.vp, ve_.vp, None, o_.vp)
                hbm("gqa: (a) two concatenation copies + rten_hip_sdpa_f32 on K, V expanded to 32 heads (what ran before)", shape, parent_route, 3 * kv_bytes)
                bsh = (C.c_int64 * 2)(2 * b_ * kv_ * p_, d_)
                hbm("gqa: (b) one strided copy of the K and V bytes (yardstick)", shape,
                    (lambda: ctx.call("rten_hip_copy_strided_b32", 2, bsh, cst, ke_.vp, ve_.vp)), 2 * kv_bytes)
                del q_, k_, v_, pk_, pv_, ok_, ov_, o_, ke_, ve_
        # first prompts of 128 / 512 / 2048 tokens: the whole call (prepare launch + GEMM, score kernel, GEMM) beside rten_hip_sdpa_f32 on the same queries with
        # K and V expanded to 32 heads and a causal [1, 1, S, S] mask -- its automatic choice (the one-kernel form up to 128 keys, else its own GEMM, softmax,
        # GEMM) and, where it covers the shape (<= 512 keys), the one-kernel form forced.  This is the comparison behind NOT extending the fused kernels here.
        for s_ in (128, 512, 2048):
            q_, k_, v_, o_ = zeros(1, s_, h_ * d_), zeros(1, s_, kv_ * d_), zeros(1, s_, kv_ * d_), zeros(1, s_, h_ * d_)
            ok_, ov_ = zeros(1, kv_, s_, d_), zeros(1, kv_, s_, d_)
            sl_, tot_ = dev(np.array([s_ - 1], np.int32)), dev(np.array([s_], np.int32))
            dims = (C.c_int32 * L.GQA_NDIMS)(1, s_, h_, kv_, d_, 0, 0, 0, 0, 0)
            st_ = (C.c_int64 * L.GQA_NSTRIDES)(s_ * h_ * d_, h_ * d_, d_, s_ * kv_ * d_, kv_ * d_, d_, s_ * kv_ * d_, kv_ * d_, d_, 0, 0, 0)
            shape = f"batch=1 seq={s_} heads={h_} kv_heads={kv_} head_size={d_}"
            flops = 4.0 * h_ * s_ * s_ * d_
            mfma("gqa: first prompt, whole call (composed path)", shape,
                 (lambda: ctx.call("rten_hip_gqa_f32", dims, st_, 0.0883883461, q_.vp, k_.vp, v_.vp, None, None, sl_.vp, tot_.vp, None, None, None, None, o_.vp, ok_.vp,
                                   ov_.vp)), flops, F32_PEAK_TF, "TFLOP/s")
            ke_, ve_ = zeros(1, h_, s_, d_), zeros(1, h_, s_, d_)
            mask_ = dev(np.triu(np.full((s_, s_), -np.inf, np.float32), 1).reshape(1, 1, s_, s_))
            sd_ = L.SdpaDesc(1, h_, s_, s_, d_, d_, s_ * h_ * d_, d_, h_ * d_, h_ * s_ * d_, s_ * d_, d_, h_ * s_ * d_, s_ * d_, d_, s_ * h_ * d_, d_, h_ * d_, s_ * s_, s_,
                             0.0883883461, 1)
            for pname, path in (("automatic", 0), ("one-kernel form forced", 2)):
                if path == 2 and s_ > 512:
                    continue
                if want("gqa:"):
                    ctx.call("rten_hip_set_sdpa_path", path)
                mfma(f"gqa: rten_hip_sdpa_f32 on 32 expanded heads with a causal mask ({pname})", shape,
                     (lambda: ctx.call("rten_hip_sdpa_f32", C.byref(sd_), q_.vp, ke_.vp, ve_.vp, mask_.vp, o_.vp)), flops, F32_PEAK_TF, "TFLOP/s")
            ctx.call("rten_hip_set_sdpa_path", 0)
            del q_, k_, v_, o_, ok_, ov_, ke_, ve_, mask_

    if args.cpu_baseline:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import bench  # the oracle is only ever touched through bench.py's cpu_baseline leg
        base = bench.cpu_op_baselines()
        for r in rows:
            key = r["op"] if r["op"] in base else f"{r['op']} {r['shape']}"
            if key in base:
                r["cpu_baseline"] = base[key]
                r["speedup_vs_cpu_port"] = round(base[key]["us"] / r["us"], 1)
    print(json.dumps({"device": ctx.device_info(), "reps": args.reps, "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
