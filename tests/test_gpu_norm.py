"""InstanceNormalization, BatchNormalization (+ activation) and LogSoftmax on the device, bit-identical to tests/norm_rules.py: the C ABI (every
InstanceNormalization path), the Python host operators, and PyTorch-exported graphs through the resident executor -- which runs the C++ host
operators of include/rten_hip_ops.hpp -- unfused, fused and captured into a hipGraph.  (The C++ operators are reached through the executor only:
tests/test_cpp_host.py builds one fixed program, and a second one would have to be compiled outside build().)"""
import os
import sys

import numpy as np
import pytest

from oracle import ref
from rten_amd import lib as L
from rten_amd import ops
from rten_amd.tensor import DeviceTensor
from tests import norm_rules as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FMAX = float(np.finfo(np.float32).max)
PATHS = {"auto": L.INSTANCE_NORM_PATH_AUTO, "streaming": L.INSTANCE_NORM_PATH_STREAMING, "resident": L.INSTANCE_NORM_PATH_RESIDENT}
CAP = L.INSTANCE_NORM_RESIDENT_MAX  # the resident form's capacity: 32768 elements (128 KiB of LDS), RTEN_HIP_INSTANCE_NORM_RESIDENT_MAX
# one case per kind (Clip with both bounds; the parameter variants are covered by tests/test_gpu_activations.py on the same device function)
ACTS = [(L.ACT_NONE, 0, 0), (L.ACT_RELU, 0, 0), (L.ACT_GELU, 0, 0), (L.ACT_SIGMOID, 0, 0), (L.ACT_SILU, 0, 0), (L.ACT_SWISH, 1.702, 0),
        (L.ACT_HARD_SIGMOID, 0.2, 0.5), (L.ACT_HARD_SWISH, 0, 0), (L.ACT_CLIP, -0.5, 1.25), (L.ACT_LEAKY_RELU, 0.1, 0), (L.ACT_ELU, 1.0, 0)]


def bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = got.view(np.int32) == want.view(np.int32)
    if not same.all():
        at = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {(~same).sum()} of {same.size} values differ, first at {at}: {got[at]!r} vs {want[at]!r}")


# ---------------------------------------------------------------------------------------------- InstanceNormalization at the ABI
def make_slices(n, c, inner, seed):
    """Mean 3, standard deviation 2 (the mean subtraction of the variance pass matters); scale / bias distinct per channel; one constant slice (var = 0)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, c, inner)) * 2 + 3).astype(np.float32)
    if n * c > 1:
        x.reshape(n * c, inner)[1] = F(1.75)
    scale = (0.5 + 0.25 * np.arange(c)).astype(np.float32)
    bias = (0.1 - 0.3 * np.arange(c)).astype(np.float32)
    return x, scale, bias


def run_instance_norm(ctx, x, scale, bias, eps, path, act=(L.ACT_NONE, 0.0, 0.0), in_place=False):
    n, c, inner = x.shape
    xd, sd, bd = (DeviceTensor.from_numpy(ctx, t) for t in (x, scale, bias))
    yd = xd if in_place else DeviceTensor(ctx, x.shape, np.float32)
    ctx.call("rten_hip_set_instance_norm_path", path)
    try:
        ctx.call("rten_hip_instance_norm_f32", n, c, inner, xd.vp, sd.vp, bd.vp, eps, act[0], float(act[1]), float(act[2]), yd.vp)
    finally:
        ctx.call("rten_hip_set_instance_norm_path", L.INSTANCE_NORM_PATH_AUTO)
    ctx.sync()
    return yd.numpy()


INNERS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000, 1024, 1025, 4099, CAP - 1, CAP, CAP + 1, 48 * 1024 + 3]


@pytest.mark.parametrize("inner", INNERS)
def test_instance_norm_every_path_gives_the_bits_of_the_rules(ctx, inner):
    """N = 2, C = 3.  1..129: every branch of the ordered reduction (masked tail only, whole 16-lane vectors, whole 64-element chunks, each plus a tail);
    1024 / 1025: the register form's limit; 4099: odd, scalar loads; CAP - 1 / CAP / CAP + 1: the resident form's capacity (above it `resident` streams);
    48 * 1024 + 3: beyond it."""
    x, scale, bias = make_slices(2, 3, inner, inner)
    want = R.instance_norm(x, scale, bias, 1e-5)
    got = {name: run_instance_norm(ctx, x, scale, bias, 1e-5, path) for name, path in PATHS.items()}
    for name, y in got.items():
        bits_equal(y, want, f"inner {inner} path {name}")


@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("inner", [100, 1028])
def test_instance_norm_row_counts_aliasing_and_epsilon(ctx, rows, inner):
    """N*C = 1 and 7 (no multiple of the register form's four rows per workgroup); y == x; epsilon given (1e-3) and the default."""
    x, scale, bias = make_slices(1, rows, inner, 50 + rows)
    for eps in (1e-5, 1e-3):
        want = R.instance_norm(x, scale, bias, eps)
        for name, path in PATHS.items():
            bits_equal(run_instance_norm(ctx, x, scale, bias, eps, path), want, f"rows {rows} inner {inner} eps {eps} {name}")
            bits_equal(run_instance_norm(ctx, x, scale, bias, eps, path, in_place=True), want, f"in place rows {rows} inner {inner} eps {eps} {name}")
    xd = DeviceTensor.from_numpy(ctx, x)
    got = ops.InstanceNormalization().run(ctx, [xd, DeviceTensor.from_numpy(ctx, scale), DeviceTensor.from_numpy(ctx, bias)])[0].numpy()  # epsilon defaulted
    bits_equal(got, R.instance_norm(x, scale, bias, 1e-5), "operator, default epsilon")


@pytest.mark.parametrize("inner", [100, 1028])
def test_instance_norm_every_activation_kind(ctx, inner):
    x, scale, bias = make_slices(2, 3, inner, 77)
    base = R.instance_norm(x, scale, bias, 1e-5)
    for kind, a, b in ACTS:
        want = R.activation(kind, base, a, b)
        for name, path in PATHS.items():
            bits_equal(run_instance_norm(ctx, x, scale, bias, 1e-5, path, act=(kind, a, b)), want, f"kind {kind} inner {inner} {name}")


def test_instance_norm_empty_inputs_and_bad_arguments(ctx):
    d = DeviceTensor.from_numpy(ctx, np.zeros(8, np.float32))
    for n, c, inner in ((0, 3, 16), (2, 0, 16), (2, 3, 0)):
        ctx.call("rten_hip_instance_norm_f32", n, c, inner, None, None, None, 1e-5, L.ACT_NONE, 0.0, 0.0, None)  # launches nothing, reads nothing
    for bad in (11, -1):
        with pytest.raises(L.HipError) as e:
            ctx.call("rten_hip_instance_norm_f32", 1, 1, 8, d.vp, d.vp, d.vp, 1e-5, bad, 0.0, 0.0, d.vp)
        assert e.value.code == L.ERR_INVALID_VALUE
        with pytest.raises(L.HipError) as e:
            ctx.call("rten_hip_batch_norm_f32_act", 1, 1, 8, d.vp, d.vp, d.vp, d.vp, d.vp, 1e-5, bad, 0.0, 0.0, d.vp)
        assert e.value.code == L.ERR_INVALID_VALUE
    with pytest.raises(L.HipError):
        ctx.call("rten_hip_set_instance_norm_path", 3)
    ctx.sync()


def test_instance_norm_path_is_part_of_the_tuning_snapshot(ctx):
    import ctypes as C
    saved = (C.c_int32 * 8)()
    ctx.call("rten_hip_set_instance_norm_path", L.INSTANCE_NORM_PATH_RESIDENT)
    try:
        ctx.call("rten_hip_tuning_save", saved)
        ctx.call("rten_hip_set_instance_norm_path", L.INSTANCE_NORM_PATH_STREAMING)
        ctx.call("rten_hip_tuning_restore", saved)
        again = (C.c_int32 * 8)()
        ctx.call("rten_hip_tuning_save", again)
        assert list(again) == list(saved) and (saved[7] >> 16) & 0xff == L.INSTANCE_NORM_PATH_RESIDENT
    finally:
        ctx.call("rten_hip_set_instance_norm_path", L.INSTANCE_NORM_PATH_AUTO)


# ---------------------------------------------------------------------------------------------- BatchNormalization
def make_bn(shape, seed):
    rng = np.random.default_rng(seed)
    c = shape[1] if len(shape) >= 2 else 1
    x = (rng.standard_normal(shape) * 2 + 1).astype(np.float32)
    scale, bias, mean = ((rng.random(c, dtype=np.float32) - F(0.5)) * F(3) for _ in range(3))
    var = rng.random(c, dtype=np.float32) * F(2) + F(0.1)
    return x, scale, bias, mean, var


def test_batch_norm_act_none_is_the_old_entry_point_and_every_kind_matches_the_rules(ctx):
    x, scale, bias, mean, var = make_bn((3, 5, 7, 9), 1)
    dev = [DeviceTensor.from_numpy(ctx, t) for t in (x, scale, bias, mean, var)]
    old, new = DeviceTensor(ctx, x.shape, np.float32), DeviceTensor(ctx, x.shape, np.float32)
    ctx.call("rten_hip_batch_norm_f32", 3, 5, 63, *[d.vp for d in dev], 1e-5, old.vp)
    ctx.call("rten_hip_batch_norm_f32_act", 3, 5, 63, *[d.vp for d in dev], 1e-5, L.ACT_NONE, 0.0, 0.0, new.vp)
    ctx.sync()
    base = R.batch_norm(x, scale, bias, mean, var, 1e-5)
    bits_equal(old.numpy(), base, "rten_hip_batch_norm_f32")
    bits_equal(new.numpy(), old.numpy(), "rten_hip_batch_norm_f32_act with ACT_NONE")
    for kind, a, b in ACTS:
        ctx.call("rten_hip_batch_norm_f32_act", 3, 5, 63, *[d.vp for d in dev], 1e-5, kind, float(a), float(b), new.vp)
        ctx.sync()
        bits_equal(new.numpy(), R.activation(kind, base, a, b), f"batch norm + kind {kind}")


def test_batch_norm_operator_one_dim_input_and_activation(ctx):
    up = lambda *ts: [DeviceTensor.from_numpy(ctx, t) for t in ts]
    x, scale, bias, mean, var = make_bn((37,), 2)  # 1-D: one channel
    got = ops.BatchNormalization().run(ctx, up(x, scale, bias, mean, var))[0].numpy()
    bits_equal(got, R.batch_norm(x, scale, bias, mean, var, 1e-5), "1-D input")
    x, scale, bias, mean, var = make_bn((4, 6), 3)  # BatchNorm1d in a head
    for act, kind, a, b in ((ops.Relu(), L.ACT_RELU, 0, 0), (ops.LeakyRelu(0.1), L.ACT_LEAKY_RELU, 0.1, 0), (ops.Clip(0.0, 6.0), L.ACT_CLIP, 0.0, 6.0), (None, L.ACT_NONE, 0, 0)):
        got = ops.BatchNormalization(epsilon=1e-3, act=act).run(ctx, up(x, scale, bias, mean, var))[0].numpy()
        bits_equal(got, R.activation(kind, R.batch_norm(x, scale, bias, mean, var, 1e-3), a, b), f"2-D input, act {kind}")
    x, scale, bias = make_slices(2, 3, 50, 4)
    got = ops.InstanceNormalization(epsilon=1e-4, act=ops.Sigmoid()).run(ctx, up(x.reshape(2, 3, 5, 10), scale, bias))[0].numpy()
    bits_equal(got, R.activation(L.ACT_SIGMOID, R.instance_norm(x, scale, bias, 1e-4)).reshape(2, 3, 5, 10), "InstanceNormalization operator + Sigmoid")


# ---------------------------------------------------------------------------------------------- LogSoftmax
@pytest.mark.parametrize("cols", [1, 5, 16, 17, 64, 97, 1024, 1025, 5000])
def test_log_softmax_columns(ctx, cols):
    """1..97: the tail branches of the 16-lane sum and every register-resident width class; 1024 / 1025: the switch to the long-row form; 5000: several
    chunks of it.  Rows 1 and 9 (9: a partly filled third workgroup of four rows)."""
    rng = np.random.default_rng(cols)
    for rows in (1, 9):
        x = (rng.standard_normal((rows, cols)) * 3).astype(np.float32)
        xd, yd = DeviceTensor.from_numpy(ctx, x), DeviceTensor(ctx, x.shape, np.float32)
        ctx.call("rten_hip_log_softmax_f32", rows, cols, xd.vp, yd.vp)
        ctx.sync()
        want = R.log_softmax(x)
        bits_equal(yd.numpy(), want, f"{rows} x {cols}")
        ctx.call("rten_hip_log_softmax_f32", rows, cols, xd.vp, xd.vp)
        ctx.sync()
        bits_equal(xd.numpy(), want, f"{rows} x {cols} in place")


def test_log_softmax_large_magnitudes_axes_and_empty(ctx):
    """x around +-80: max is large and ln(sum) small, where (x - max) - ln(sum) and x - (max + ln(sum)) differ."""
    rng = np.random.default_rng(3)
    x = (np.where(rng.random((6, 40)) < 0.5, 80.0, -80.0) + rng.standard_normal((6, 40))).astype(np.float32)
    got = ops.LogSoftmax().run(ctx, [DeviceTensor.from_numpy(ctx, x)])[0].numpy()
    want = R.log_softmax(x)
    bits_equal(got, want, "large magnitudes")
    mx = x.max(axis=1, keepdims=True)
    one_subtraction = (x - (mx + np.array([[R.correctly_rounded_ln(R.log_softmax_row(r)[1])] for r in x], np.float32))).astype(np.float32)
    assert not np.array_equal(one_subtraction, want)  # the data does tell the two forms apart
    t = (rng.standard_normal((3, 5, 7)) * 2).astype(np.float32)
    for axis in (0, 1, -1):
        got = ops.LogSoftmax(axis=axis).run(ctx, [DeviceTensor.from_numpy(ctx, t)])[0].numpy()
        bits_equal(got, R.log_softmax(t, axis), f"axis {axis} of [3, 5, 7]")
    ctx.call("rten_hip_log_softmax_f32", 0, 5, None, None)
    ctx.call("rten_hip_log_softmax_f32", 5, 0, None, None)
    ctx.sync()


# ---------------------------------------------------------------------------------------------- exported graphs through the resident executor
def _te():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export as te
    return te


def run_model(tmp_path, data, x, out_name, *flags, sizes=("batch",)):
    from tests.test_graph_executor import run_cli
    model, xin, yout = tmp_path / "m.onnx", tmp_path / "x.bin", tmp_path / "y.bin"
    model.write_bytes(data)
    xin.write_bytes(np.ascontiguousarray(x, np.float32).tobytes())
    dims = {"batch": x.shape[0], "width": x.shape[-1]}
    args = [a for s in sizes for a in ("-s", f"{s}={dims[s]}")]
    out = run_cli(*flags, *args, "--input", f"x={xin}", "--dump", f"{out_name}={yout}", str(model))
    assert out.returncode == 0, out.stderr + out.stdout
    return np.fromfile(yout, np.float32), out.stdout


MODES = (("--no-fuse",), (), ("--graph", "-n", "3"))


def three_ways(tmp_path, data, x, out_name, shape, sizes=("batch",)):
    runs = [run_model(tmp_path, data, x, out_name, *flags, sizes=sizes) for flags in MODES]
    assert "Captured the plan into a hipGraph" in runs[2][1]
    return [r[0].reshape(shape) for r in runs], runs[1][1]


def preact_expected(module, x):
    """The pre-activation net one graph node at a time: oracle convolution / pool / GEMM, the rules for the BatchNormalization (+ activation) nodes."""
    p = {k: v.detach().numpy() for k, v in module.state_dict().items()}
    bn = lambda t, k: R.batch_norm(t, p[k + ".weight"], p[k + ".bias"], p[k + ".running_mean"], p[k + ".running_var"], 1e-5)
    y = ref.conv2d_f32(x, p["stem.weight"], p["stem.bias"], pads=(1, 1, 1, 1))
    t = R.activation(L.ACT_RELU, bn(y, "bn1"))
    y = ref.add(y, ref.conv2d_f32(t, p["conv1.weight"], p["conv1.bias"], pads=(1, 1, 1, 1))).reshape(y.shape)
    y = ref.max_pool(y, (2, 2), (2, 2))
    t = R.activation(L.ACT_LEAKY_RELU, bn(y, "bn2"), 0.1)
    y = ref.conv2d_f32(t, p["conv2.weight"], p["conv2.bias"])
    g = bn(ref.global_average_pool(y).reshape(y.shape[0], -1), "bn3")
    c0 = np.broadcast_to(p["fc.bias"], (g.shape[0], p["fc.weight"].shape[0])).astype(np.float32)
    return ref.gemm_f32(g, p["fc.weight"].T, c=c0, alpha=1.0, beta=1.0)  # Gemm(transB=1, alpha=1, beta=1, C=bias)


@pytest.mark.parametrize("dynamic", [False, True])
def test_exported_preact_net_node_by_node_fused_and_captured(tmp_path, dynamic):
    te = _te()
    module = te.preact_module(seed=3)
    data = te.preact_onnx(module, dynamic=dynamic)
    for batch in [2] + ([3] if dynamic else []):
        x = (np.random.default_rng(batch).random((batch, 3, 16, 16), dtype=np.float32) - F(0.5)).astype(np.float32)
        want = preact_expected(module, x)
        got, stdout = three_ways(tmp_path, data, x, "logits", want.shape, sizes=("batch",) if dynamic else ())
        for y, mode in zip(got, MODES):
            bits_equal(y, want, f"preact batch {batch} {' '.join(mode) or 'fused'}")


@pytest.mark.parametrize("dynamic", [False, True])
def test_exported_recognizer_with_log_softmax_head(tmp_path, dynamic):
    from tests.test_gpu_rnn import expected_output
    te = _te()
    module = te.recognizer_module("gru", True, 1, seed=4, log_softmax=True)
    data = te.recognizer_onnx(module, dynamic=dynamic)
    for batch, width in [(2, 12)] + ([(3, 7)] if dynamic else []):
        x = (np.random.default_rng(batch * 100 + width).random((batch, 1, 8, width), dtype=np.float32) - F(0.5)).astype(np.float32)
        want = R.log_softmax(expected_output(module, "gru", True, 1, x), -1)
        got, _ = three_ways(tmp_path, data, x, "y", want.shape, sizes=("batch", "width") if dynamic else ())
        for y, mode in zip(got, MODES):
            bits_equal(y, want, f"recogniser {batch}x{width} {' '.join(mode) or 'fused'}")


def generator_expected(module, x):
    """The generator one graph node at a time: oracle convolutions / transposed convolution / tanh, the rules for InstanceNormalization (+ Relu)."""
    p = {k: v.detach().numpy() for k, v in module.state_dict().items()}
    relu = lambda t: R.activation(L.ACT_RELU, t)
    inorm = lambda t, k: R.instance_norm(t, p[k + ".weight"], p[k + ".bias"], 1e-5)
    conv = lambda t, k, s=1: ref.conv2d_f32(t, p[k + ".weight"], p[k + ".bias"], pads=(1, 1, 1, 1), strides=(s, s))
    y = relu(inorm(conv(x, "body.0"), "body.1"))
    y = relu(inorm(conv(y, "body.3", 2), "body.4"))
    for b in ("body.6.body.", "body.7.body."):
        t = relu(inorm(conv(y, b + "0"), b + "1"))
        y = ref.add(y, inorm(conv(t, b + "3"), b + "4")).reshape(y.shape)
    y = ref.conv_transpose2d_f32(y, p["body.8.weight"], p["body.8.bias"], padding=(1, 1, 1, 1), strides=(2, 2), output_padding=(1, 1))
    return ref.tanh(conv(relu(inorm(y, "body.9")), "body.11"))


@pytest.mark.parametrize("dynamic", [False, True])
def test_exported_generator_fused_unfused_captured_and_against_torch(tmp_path, dynamic):
    import torch
    te = _te()
    module = te.generator_module(seed=5)
    data = te.generator_onnx(module, dynamic=dynamic)
    for batch in [2] + ([3] if dynamic else []):
        x = (np.random.default_rng(batch).random((batch, 3, 16, 16), dtype=np.float32) - F(0.5)).astype(np.float32)
        got, stdout = three_ways(tmp_path, data, x, "y", x.shape, sizes=("batch",) if dynamic else ())
        bits_equal(got[0], generator_expected(module, x), "generator --no-fuse vs the oracle composition")
        bits_equal(got[1], got[0], "generator fused vs --no-fuse")
        bits_equal(got[2], got[0], "generator --graph vs --no-fuse")
        with torch.no_grad():
            t = module(torch.from_numpy(x)).numpy()
        diff = np.abs(got[1] - t).max()
        print(f"generator batch {batch}: max |device - torch| = {diff:.3e}")
        assert diff <= 1e-4  # expect_eq_1e4: the reference's bar for these operators


def test_loading_through_the_executor_names_the_refused_node(tmp_path):
    from tests.test_graph_executor import run_cli
    from tests.test_norm_ops import _bn_model
    p = tmp_path / "bad.onnx"
    p.write_bytes(_bn_model({}, ("y", "rm")))
    out = run_cli(str(p))
    assert out.returncode == 1 and "bn_node" in out.stderr and "running_mean" in out.stderr, out.stderr
