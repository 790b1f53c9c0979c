"""Sigmoid / Silu / Swish / HardSigmoid / HardSwish / Clip / LeakyRelu / Elu on the device: the element-wise kernel, the epilogues of
the f32 convolution / depthwise / GEMM / GEMV kernels, and whole graphs through rten_hip_run.  Expected values are numpy restatements
of the reference's formulas (rten-vecmath/src/exp.rs:201-275, relu.rs:13-25, src/ops/unary_elementwise.rs:248-303,437-471), one
rounded f32 operation at a time, on the oracle's exp."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import ref
from rten_amd import lib as L
from rten_amd import ops
from rten_amd.tensor import DeviceTensor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FMAX = float(np.finfo(np.float32).max)


def np_act(kind, x, a=0.0, b=0.0):
    x = np.asarray(x, np.float32)
    a, b = F(a), F(b)
    one, zero = F(1), F(0)
    with np.errstate(all="ignore"):
        def sigmoid(v):
            return one / (one + ref.exp(-v))

        def clamp01(v):  # f32::clamp(v, 0, 1): NaN and -0 pass through
            v = np.where(v < zero, zero, v)
            return np.where(v > one, one, v).astype(np.float32)
        if kind == L.ACT_NONE:
            return x.copy()
        if kind == L.ACT_RELU:
            return ref.relu(x)
        if kind == L.ACT_GELU:
            return ref.gelu(x)
        if kind == L.ACT_SIGMOID:
            return sigmoid(x)
        if kind == L.ACT_SILU:
            return x / (one + ref.exp(-x))
        if kind == L.ACT_SWISH:
            return x * sigmoid(x * a)
        if kind == L.ACT_HARD_SIGMOID:
            return clamp01(a * x + b)
        if kind == L.ACT_HARD_SWISH:
            return x * clamp01((one / F(6)) * x + F(0.5))
        if kind == L.ACT_CLIP:
            y = np.where(x > a, x, a)
            return np.where(y < b, y, b).astype(np.float32)
        if kind == L.ACT_LEAKY_RELU:
            return np.where(x < zero, x * a, x).astype(np.float32)
        if kind == L.ACT_ELU:
            return np.where(x >= zero, x, a * (ref.exp(x) - one)).astype(np.float32)
    raise ValueError(kind)


# every kind, with the parameter cases that matter (Clip: both bounds, no min, no max, min > max, -inf bound)
CASES = [(L.ACT_RELU, 0, 0), (L.ACT_GELU, 0, 0), (L.ACT_SIGMOID, 0, 0), (L.ACT_SILU, 0, 0), (L.ACT_SWISH, 1.702, 0), (L.ACT_SWISH, 1.0, 0),
         (L.ACT_HARD_SIGMOID, 0.2, 0.5), (L.ACT_HARD_SIGMOID, 1.0 / 6.0, 0.5), (L.ACT_HARD_SWISH, 0, 0), (L.ACT_CLIP, 0.0, 6.0),
         (L.ACT_CLIP, -FMAX, 6.0), (L.ACT_CLIP, 0.0, FMAX), (L.ACT_CLIP, 3.0, -1.0), (L.ACT_CLIP, -np.inf, 0.25), (L.ACT_LEAKY_RELU, 0.01, 0),
         (L.ACT_LEAKY_RELU, 0.1, 0), (L.ACT_ELU, 1.0, 0), (L.ACT_ELU, 0.5, 0)]
EPI_CASES = [c for c in CASES if c[0] not in (L.ACT_RELU, L.ACT_GELU)]  # the two old kinds have their own epilogue tests


def assert_bits(got, want, what=""):
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    bad = np.flatnonzero(got[~nan].view(np.int32) != want[~nan].view(np.int32))
    if bad.size:
        i = bad[0]
        x = (got[~nan][i], want[~nan][i])
        raise AssertionError(f"{what}: {bad.size} elements differ, first got {x[0]!r} want {x[1]!r}")


def edge_values():
    tiny = np.array([1, 3, 0x7fffff], np.int32).view(np.float32)  # denormals
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, FMAX, -FMAX, 104.0, -104.0, 103.99, -103.99, 104.01, -104.01, 88.7, -88.7, 87.3, -87.3,
         1.0, -1.0, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0, 6.0000005, 2.9999998, 1e-7, -1e-7, 1e-30, -1e-30, 20.0, -20.0, 50.0, -50.0]
    return np.concatenate([np.array(v, np.float32), tiny, -tiny])


def run_act(ctx, kind, a, b, x, in_place=False, offset=0):
    """rten_hip_activation_f32 on x placed `offset` floats into its device buffer (offset 1: not 16-byte aligned)."""
    buf = DeviceTensor.from_numpy(ctx, np.concatenate([np.zeros(offset, np.float32), x]))
    xd = DeviceTensor(ctx, (x.size,), np.float32, ptr=buf.ptr + 4 * offset, keepalive=buf)
    yd = xd if in_place else DeviceTensor(ctx, (x.size + offset,), np.float32)
    yp = yd.ptr if in_place else yd.ptr + 4 * offset
    ctx.call("rten_hip_activation_f32", kind, a, b, x.size, xd.vp if x.size else None, C.c_void_p(yp) if x.size else None)
    ctx.sync()
    out = yd.numpy()
    return out if in_place else out[offset:]


def test_activation_kernel_edge_values_every_kind(ctx):
    rng = np.random.default_rng(1)
    x = np.concatenate([edge_values(), (rng.standard_normal(4000) * 8).astype(np.float32)])
    for kind, a, b in CASES:
        want = np_act(kind, x, a, b)
        assert_bits(run_act(ctx, kind, a, b, x), want, f"kind {kind} ({a}, {b})")


def test_activation_kernel_lengths_alignment_and_in_place(ctx):
    rng = np.random.default_rng(2)
    big = (rng.standard_normal(12_500_003) * 6).astype(np.float32)
    for kind, a, b in ((L.ACT_SILU, 0, 0), (L.ACT_CLIP, 0.0, 6.0), (L.ACT_HARD_SWISH, 0, 0), (L.ACT_ELU, 1.0, 0)):
        for n in (0, 1, 3, 4097):
            x = big[:n].copy()
            for offset in (0, 1):
                assert_bits(run_act(ctx, kind, a, b, x, offset=offset), np_act(kind, x, a, b), f"kind {kind} n {n} offset {offset}")
                assert_bits(run_act(ctx, kind, a, b, x, in_place=True, offset=offset), np_act(kind, x, a, b), f"in place kind {kind} n {n}")
    for kind, a, b in CASES:
        assert_bits(run_act(ctx, kind, a, b, big), np_act(kind, big, a, b), f"12.5 M kind {kind}")
    assert_bits(run_act(ctx, L.ACT_SIGMOID, 0, 0, big, in_place=True, offset=1), np_act(L.ACT_SIGMOID, big), "12.5 M in place unaligned")


def test_unknown_kind_is_invalid_value(ctx):
    xd = DeviceTensor.from_numpy(ctx, np.zeros(8, np.float32))
    for fn, args in (("rten_hip_activation_f32", (11, 0.0, 0.0, 8, xd.vp, xd.vp)), ("rten_hip_activation_f32", (-1, 0.0, 0.0, 8, xd.vp, xd.vp))):
        with pytest.raises(L.HipError) as e:
            ctx.call(fn, *args)
        assert e.value.code == L.ERR_INVALID_VALUE
    d = L.gemm_desc(4, 4, 2, 2, 1, 4, 1, 4)
    with pytest.raises(L.HipError) as e:
        ctx.call("rten_hip_gemm_f32_act", C.byref(d), xd.vp, xd.vp, None, 12, 0.0, 0.0, xd.vp)
    assert e.value.code == L.ERR_INVALID_VALUE


def test_python_operators(ctx):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((2, 3, 5, 7)) * 4).astype(np.float32)
    xd = DeviceTensor.from_numpy(ctx, x)
    for op, kind, a, b in ((ops.Sigmoid(), L.ACT_SIGMOID, 0, 0), (ops.Silu(), L.ACT_SILU, 0, 0), (ops.Swish(), L.ACT_SWISH, 1.0, 0),
                           (ops.HardSigmoid(), L.ACT_HARD_SIGMOID, 0.2, 0.5), (ops.HardSwish(), L.ACT_HARD_SWISH, 0, 0),
                           (ops.LeakyRelu(), L.ACT_LEAKY_RELU, 0.01, 0), (ops.Elu(), L.ACT_ELU, 1.0, 0), (ops.Clip(), L.ACT_CLIP, -FMAX, FMAX),
                           (ops.Clip(-1.0, 2.0), L.ACT_CLIP, -1.0, 2.0)):
        assert_bits(op.run(ctx, [xd])[0].numpy(), np_act(kind, x, a, b), type(op).__name__)
    lo, hi = DeviceTensor.from_numpy(ctx, np.array(0.0, np.float32)), DeviceTensor.from_numpy(ctx, np.array(6.0, np.float32))
    assert_bits(ops.Clip().run(ctx, [xd, lo, hi])[0].numpy(), np_act(L.ACT_CLIP, x, 0.0, 6.0), "Clip with input bounds")
    assert_bits(ops.Clip().run(ctx, [xd, None, hi])[0].numpy(), np_act(L.ACT_CLIP, x, -FMAX, 6.0), "Clip without min")
    with pytest.raises(ops.OpError) as e:
        ops.Clip().run(ctx, [xd, DeviceTensor.from_numpy(ctx, np.zeros(2, np.float32))])
    assert e.value.kind == "InvalidValue"


# ---------------------------------------------------------------------------------------------------- epilogues
def conv(ctx, x, w, bias, pads, act, strides=(1, 1), groups=1, residual=None, packed=True, variant=None):
    op = ops.Conv(groups=groups, padding=list(pads), strides=list(strides), act=ops_act(*act) if act else None)
    xd, wd = DeviceTensor.from_numpy(ctx, x), DeviceTensor.from_numpy(ctx, w)
    pw = op.prepack(ctx, wd, op._geometry(ctx, x.shape, w.shape)) if packed else None
    ins = [xd, wd, DeviceTensor.from_numpy(ctx, bias) if bias is not None else None]
    if residual is not None:
        ins.append(DeviceTensor.from_numpy(ctx, residual))
    if variant is not None:
        ctx.set_gemm_variant(variant)
    try:
        return op.run(ctx, ins, packed_weight=pw)[0].numpy()
    finally:
        ctx.set_gemm_variant(-1)


def ops_act(kind, a, b):
    o = ops._Activation(a, b)
    o.kind = kind
    return o


def gemm(ctx, a, b, bias, act, variant=None):
    M, K = a.shape
    N = b.shape[1]
    ad, bd = DeviceTensor.from_numpy(ctx, a), DeviceTensor.from_numpy(ctx, b)
    cd = DeviceTensor.from_numpy(ctx, np.full((M, N), np.nan, np.float32))
    biasd = DeviceTensor.from_numpy(ctx, bias) if bias is not None else None
    d = L.gemm_desc(M, N, K, K, 1, N, 1, N, bias_kind=L.BIAS_PER_COL if bias is not None else L.BIAS_NONE)
    if variant is not None:
        ctx.set_gemm_variant(variant)
    try:
        ctx.call("rten_hip_gemm_f32_act", C.byref(d), ad.vp, bd.vp, biasd.vp if biasd else None, act[0], act[1], act[2], cd.vp)
    finally:
        ctx.set_gemm_variant(-1)
    return cd.numpy()


def test_conv_epilogue_every_kind_every_variant(ctx):
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((2, 32, 14, 14))).astype(np.float32)
    w = (rng.standard_normal((48, 32, 3, 3)) * 0.1).astype(np.float32)
    bias = rng.standard_normal(48).astype(np.float32)
    base = ref.conv2d_f32(x, w, bias, pads=(1, 1, 1, 1))
    for v in range(ctx.lib.rten_hip_num_gemm_variants()):
        for case in EPI_CASES:
            assert_bits(conv(ctx, x, w, bias, (1, 1, 1, 1), case, variant=v), np_act(case[0], base, case[1], case[2]), f"variant {v} act {case}")
    # unpacked weights and a pointwise convolution (the N4 loader)
    w1 = (rng.standard_normal((24, 32, 1, 1)) * 0.2).astype(np.float32)
    base1 = ref.conv2d_f32(x, w1, None)
    for case in EPI_CASES:
        assert_bits(conv(ctx, x, w1, None, (0, 0, 0, 0), case), np_act(case[0], base1, case[1], case[2]), f"pointwise {case}")
        assert_bits(conv(ctx, x, w, bias, (1, 1, 1, 1), case, packed=False), np_act(case[0], base, case[1], case[2]), f"unpacked {case}")


def test_conv_epilogue_with_residual_and_exact_split_k(ctx):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 256, 7, 7)).astype(np.float32)
    w = (rng.standard_normal((64, 256, 3, 3)) * 0.03).astype(np.float32)
    bias = rng.standard_normal(64).astype(np.float32)
    res = rng.standard_normal((2, 64, 7, 7)).astype(np.float32)
    with_res = ref.conv2d_f32(x, w, bias, pads=(1, 1, 1, 1), residual=res)
    plain = ref.conv2d_f32(x, w, bias, pads=(1, 1, 1, 1))
    try:
        for mode, groups in ((3, 1), (2, 2), (2, 3), (2, 64)):
            ctx.call("rten_hip_set_gemm_split", mode, groups)
            for case in ((L.ACT_SILU, 0, 0), (L.ACT_CLIP, 0.0, 6.0), (L.ACT_HARD_SWISH, 0, 0), (L.ACT_ELU, 0.5, 0)):
                assert_bits(conv(ctx, x, w, bias, (1, 1, 1, 1), case, residual=res), np_act(case[0], with_res, case[1], case[2]), f"split {mode},{groups} residual {case}")
                assert_bits(conv(ctx, x, w, bias, (1, 1, 1, 1), case), np_act(case[0], plain, case[1], case[2]), f"split {mode},{groups} {case}")
    finally:
        ctx.call("rten_hip_set_gemm_split", 3, 1)


def test_conv_relu_flag_is_refused_by_the_act_entry(ctx):
    x = DeviceTensor.from_numpy(ctx, np.zeros((1, 4, 4, 4), np.float32))
    w = DeviceTensor.from_numpy(ctx, np.zeros((4, 4, 1, 1), np.float32))
    d = ops.Conv()._geometry(ctx, (1, 4, 4, 4), (4, 4, 1, 1))
    with pytest.raises(L.HipError) as e:
        ctx.call("rten_hip_conv2d_f32_act", C.byref(d), x.vp, w.vp, 0, None, None, L.CONV_RELU, L.ACT_SILU, 0.0, 0.0, x.vp)
    assert e.value.code == L.ERR_INVALID_VALUE


def test_depthwise_epilogue_three_kernel_forms(ctx):
    rng = np.random.default_rng(6)
    for shape, k, stride, pad in (((2, 32, 16, 16), 3, 1, 1),   # the streaming 3x3 stride-1 kernel
                                  ((2, 24, 15, 17), 3, 2, 1),   # four rows per thread (stride 2)
                                  ((2, 16, 9, 9), 5, 1, 2)):    # the generic kernel
        c = shape[1]
        x = rng.standard_normal(shape).astype(np.float32)
        w = (rng.standard_normal((c, 1, k, k)) * 0.3).astype(np.float32)
        bias = rng.standard_normal(c).astype(np.float32)
        base = ref.conv2d_f32(x, w, bias, pads=(pad,) * 4, strides=(stride, stride), groups=c)
        res = rng.standard_normal(base.shape).astype(np.float32)
        with_res = ref.conv2d_f32(x, w, bias, pads=(pad,) * 4, strides=(stride, stride), groups=c, residual=res)
        for case in CASES:
            got = conv(ctx, x, w, bias, (pad,) * 4, case, strides=(stride, stride), groups=c, packed=False)
            assert_bits(got, np_act(case[0], base, case[1], case[2]), f"depthwise {shape} {case}")
        for case in ((L.ACT_SILU, 0, 0), (L.ACT_CLIP, 0.0, 6.0)):
            got = conv(ctx, x, w, bias, (pad,) * 4, case, strides=(stride, stride), groups=c, residual=res, packed=False)
            assert_bits(got, np_act(case[0], with_res, case[1], case[2]), f"depthwise residual {shape} {case}")


def test_gemm_and_gemv_epilogue_every_kind(ctx):
    rng = np.random.default_rng(7)
    a = (rng.standard_normal((200, 300))).astype(np.float32)
    b = (rng.standard_normal((300, 136)) * 0.1).astype(np.float32)
    bias = rng.standard_normal(136).astype(np.float32)
    base = ref.gemm_f32(a, b, bias=bias, bias_kind=ref.BIAS_PER_COL)
    for v in range(ctx.lib.rten_hip_num_gemm_variants()):
        for case in EPI_CASES:
            assert_bits(gemm(ctx, a, b, bias, case, variant=v), np_act(case[0], base, case[1], case[2]), f"variant {v} {case}")
    try:
        for mode, groups in ((2, 2), (2, 64)):
            ctx.call("rten_hip_set_gemm_split", mode, groups)
            for case in ((L.ACT_SILU, 0, 0), (L.ACT_HARD_SIGMOID, 0.2, 0.5)):
                assert_bits(gemm(ctx, a, b, bias, case), np_act(case[0], base, case[1], case[2]), f"split {mode},{groups} {case}")
    finally:
        ctx.call("rten_hip_set_gemm_split", 3, 1)
    # one row: the reference's gemv order (m == 1), and a few rows (the small-M kernel)
    for m in (1, 5):
        a1 = a[:m].copy()
        base1 = ref.gemm_f32(a1, b, bias=bias, bias_kind=ref.BIAS_PER_COL)
        for case in CASES:
            assert_bits(gemm(ctx, a1, b, bias, case), np_act(case[0], base1, case[1], case[2]), f"m {m} {case}")
    # through the operator (act on MatMul / FusedMatMul)
    ad, bd = DeviceTensor.from_numpy(ctx, a), DeviceTensor.from_numpy(ctx, b)
    assert_bits(ops.MatMul(act=ops.Silu()).run(ctx, [ad, bd])[0].numpy(), np_act(L.ACT_SILU, ref.matmul_f32(a, b)), "MatMul act")
    got = ops.FusedMatMul(act=ops.Clip(0.0, 6.0)).run(ctx, [ad, bd, DeviceTensor.from_numpy(ctx, bias)])[0].numpy()
    assert_bits(got, np_act(L.ACT_CLIP, ref.matmul_f32(a, b, bias=bias), 0.0, 6.0), "FusedMatMul act")


# ---------------------------------------------------------------------------------------------------- graphs
def _cli():
    from tests.test_graph_executor import run_cli
    return run_cli


def _run(tmp_path, model_bytes, inputs, out_name, *extra):
    p = tmp_path / "m.onnx"
    p.write_bytes(model_bytes)
    args = []
    for name, arr in inputs.items():
        f = tmp_path / f"{name}.bin"
        arr.astype(np.float32).tofile(f)
        args += ["--input", f"{name}={f}"]
    yout = tmp_path / "y.bin"
    batch = next(iter(inputs.values())).shape[0]
    r = _cli()("-s", f"batch={batch}", *args, "--dump", f"{out_name}={yout}", *extra, str(p))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.fromfile(yout, np.float32), r.stdout


def test_pytorch_exported_mobile_network(tmp_path):
    """ReLU6 / Hardswish / Hardsigmoid and Sigmoid squeeze-excite / SiLU / QuickGELU / LeakyReLU / ELU as PyTorch exports them, at batch 3:
    the same bits fused, unfused and replayed from a captured graph; the fused plan runs the convolutions' activations in their epilogues;
    torch's CPU forward agrees to f32 accumulation-order tolerance."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export as te
    model = te.mobile_module()
    data = te.mobile_onnx(model)
    x = np.random.default_rng(8).standard_normal((3, 3, 32, 32)).astype(np.float32)
    fused, log = _run(tmp_path, data, {"x": x}, "logits", "-t")
    unfused, _ = _run(tmp_path, data, {"x": x}, "logits", "--no-fuse")
    graph, _ = _run(tmp_path, data, {"x": x}, "logits", "--graph", "-n", "2")
    assert_bits(unfused, fused, "--no-fuse")
    assert_bits(graph, fused, "--graph")
    for kind in ("Conv+Clip", "Conv+Silu", "Conv+Elu", "Conv+LeakyRelu", "Conv+HardSigmoid", "Conv+Relu"):
        assert kind in log, (kind, log[-3000:])
    assert "Swish" in log and "Sigmoid" in log
    steps = [l.split() for l in log.splitlines()]
    assert not any(s and s[0] == "Clip" for s in steps), "a standalone Clip step is left"
    with torch.no_grad():
        want = model(torch.from_numpy(x)).numpy()
    np.testing.assert_allclose(fused.reshape(want.shape), want, rtol=1e-4, atol=1e-4)


def test_conv_hardswish_and_clip_inputs_graph(tmp_path):
    """Conv -> HardSwish fuses (Conv+HardSwish); a Clip whose min is an empty name and max an initializer runs standalone with those bounds;
    LeakyRelu / Elu take the reference's default alpha."""
    from rten_amd import onnx_writer as ow
    rng = np.random.default_rng(9)
    x = rng.standard_normal((2, 8, 10, 10)).astype(np.float32)
    w = (rng.standard_normal((12, 8, 3, 3)) * 0.3).astype(np.float32)
    b = rng.standard_normal(12).astype(np.float32)
    nodes = [ow.node("Conv", ["x", "w", "b"], ["c"], name="conv", kernel_shape=[3, 3], pads=[1, 1, 1, 1]),
             ow.node("HardSwish", ["c"], ["h"], name="hs"),
             ow.node("Clip", ["h", "", "mx"], ["k"], name="clip"),
             ow.node("LeakyRelu", ["k"], ["l"], name="leaky"),
             ow.node("Elu", ["l"], ["y"], name="elu")]
    m = ow.model(nodes, [ow.value_info("x", ow.FLOAT, ["batch", 8, 10, 10])], [ow.value_info("y", ow.FLOAT, ["batch", 12, 10, 10])],
                 [ow.tensor("w", w), ow.tensor("b", b), ow.tensor("mx", np.array(0.75, np.float32))])
    base = ref.conv2d_f32(x, w, b, pads=(1, 1, 1, 1))
    want = np_act(L.ACT_ELU, np_act(L.ACT_LEAKY_RELU, np_act(L.ACT_CLIP, np_act(L.ACT_HARD_SWISH, base), -FMAX, 0.75), 0.01), 1.0)
    got, log = _run(tmp_path, m, {"x": x}, "y", "-t")
    assert_bits(got, want, "fused")
    assert "Conv+HardSwish" in log, log[-2000:]
    got2, _ = _run(tmp_path, m, {"x": x}, "y", "--no-fuse")
    assert_bits(got2, want, "unfused")


def test_swiglu_block_runs_as_fused_matmul_silu(tmp_path):
    """The SwiGLU MLP of LLM decoders: Mul(Silu(x Wg), x Wu) with Silu spelled Sigmoid + Mul -> SiluFusion, then the gate
    projection's epilogue (FusedMatMul+Silu)."""
    from rten_amd import onnx_writer as ow
    rng = np.random.default_rng(10)
    x = rng.standard_normal((2, 8, 64)).astype(np.float32)
    wg = (rng.standard_normal((64, 96)) * 0.2).astype(np.float32)
    wu = (rng.standard_normal((64, 96)) * 0.2).astype(np.float32)
    nodes = [ow.node("MatMul", ["x", "wg"], ["g"], name="gate"),
             ow.node("Sigmoid", ["g"], ["s"], name="sig"),
             ow.node("Mul", ["g", "s"], ["a"], name="silu"),
             ow.node("MatMul", ["x", "wu"], ["u"], name="up"),
             ow.node("Mul", ["a", "u"], ["y"], name="glu")]
    m = ow.model(nodes, [ow.value_info("x", ow.FLOAT, ["batch", 8, 64])], [ow.value_info("y", ow.FLOAT, ["batch", 8, 96])],
                 [ow.tensor("wg", wg), ow.tensor("wu", wu)])
    want = np_act(L.ACT_SILU, ref.matmul_f32(x, wg)) * ref.matmul_f32(x, wu)
    for extra in (("-t",), ("--no-fuse",), ("--graph", "-n", "2")):
        got, log = _run(tmp_path, m, {"x": x}, "y", *extra)
        assert_bits(got, want, str(extra))
        if extra == ("-t",):
            assert "FusedMatMul+Silu" in log, log[-2000:]
