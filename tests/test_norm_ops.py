"""InstanceNormalization / BatchNormalization / LogSoftmax without a GPU: the expected values (tests/norm_rules.py) against the reference's own
test literals, the bound on the one deliberate divergence (ln of the exp-sum), the host operators' validation, and what the ONNX loader accepts,
fuses and refuses (through rten_hip_run --parse-only)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from tests import norm_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "norm_reference.json")))  # literals of src/ops/norm.rs:930-1075,1266-1299
F = np.float32


def _arr(v, shape=None):
    a = np.asarray(v, np.float32)
    return a.reshape(shape) if shape is not None else a


# ---------------------------------------------------------------------------------------------- the rules against the reference's literals
def test_instance_norm_rules_reproduce_the_reference_literals():
    """expect_eq_1e4 = expect_equal_with_tolerance(.., atol 1e-4, rtol 0) (src/ops/mod.rs:407-412)."""
    g = GOLDEN["instance_normalization"]
    y = R.instance_norm(_arr(g["input"]["data"], g["input"]["shape"]), _arr(g["scale"]), _arr(g["bias"]))
    err = np.abs(y.ravel().astype(np.float64) - np.asarray(g["expected"]))
    print("largest |diff|", err.max())
    assert (err <= 1e-4).all()


@pytest.mark.parametrize("case", range(4))
def test_log_softmax_rules_reproduce_the_reference_literals(case):
    g = GOLDEN["log_softmax"][case]
    y = R.log_softmax(_arr(g["input"], g["shape"]), g["axis"])
    err = np.abs(y.ravel().astype(np.float64) - np.asarray(g["expected"]))
    print("largest |diff|", err.max())
    assert (err <= 1e-4).all()


@pytest.mark.parametrize("case", range(4))
def test_batch_norm_rules_reproduce_the_reference_formula(case):
    """test_batch_norm (norm.rs:930-987): expected = (x - mean) / sqrt(var + eps) * scale + bias in f32, compared with expect_equal's
    defaults: |a - b| <= 1e-8 + 1e-5 * |b|.  A 1-D input has one channel."""
    g = GOLDEN["batch_norm"]
    inp = g["inputs"][case]
    x = _arr(inp["data"], inp["shape"])
    n = 2 if x.ndim >= 2 else 1
    scale, bias, mean, var = (_arr(g[k][:n]) for k in ("scale", "bias", "mean", "var"))
    eps = F(g["epsilon"])
    y = R.batch_norm(x, scale, bias, mean, var, float(eps))
    flat = x.ravel()
    ch = (lambda i: i) if x.ndim >= 2 else (lambda i: 0)
    want = np.array([(flat[i] - mean[ch(i)]) / np.sqrt(var[ch(i)] + eps) * scale[ch(i)] + bias[ch(i)] for i in range(flat.size)], np.float32)
    err = np.abs(y.ravel().astype(np.float64) - want)
    assert y.shape == x.shape
    assert (err <= 1e-8 + 1e-5 * np.abs(want.astype(np.float64))).all(), (y, want)


def test_libm_logf_divergence_is_one_ulp_of_the_logarithm():
    """ln(sum) is where "the reference's bits" are not defined: it calls the host's logf.  Over 2000 seeded rows (5, 17, 97 and 300 columns), glibc's
    logf differs from the correctly rounded logarithm on 21 rows (1.05 %), never by more than one ulp of ln(sum).  The output y = (x - max) - ln(sum) is
    rounded once more, on its own grid: where |y| >= 2 |ln(sum)| that grid is coarser, and a one-ulp change of ln(sum) moves y by either nothing or one
    step of y's grid (measured: up to 8 ulps of ln(sum), on 4 rows).  So the bound per element is one ulp of ln(sum) or one ulp of y, whichever is
    larger; the bound on the logarithm itself is one ulp."""
    libm = C.CDLL("libm.so.6")
    libm.logf.restype, libm.logf.argtypes = C.c_float, [C.c_float]
    ln_libm = lambda s: F(libm.logf(float(s)))
    rng = np.random.default_rng(7)
    rows = differing = 0
    for cols in (5, 17, 97, 300):
        for _ in range(500):
            x = (rng.standard_normal(cols) * 3).astype(np.float32)
            y, s = R.log_softmax_row(x)
            y_libm, _ = R.log_softmax_row(x, ln_libm)
            lg = R.correctly_rounded_ln(s)
            u = float(np.spacing(np.abs(lg)))
            assert abs(float(ln_libm(s)) - float(lg)) <= u
            d = np.abs(y.astype(np.float64) - y_libm.astype(np.float64))
            assert (d <= np.maximum(u, np.spacing(np.abs(y)).astype(np.float64))).all()
            rows += 1
            differing += bool((d > 0).any())
    print(f"{differing} of {rows} rows differ")
    assert differing < rows // 10


# ---------------------------------------------------------------------------------------------- host operators
class _Shape:
    """An operand as the validation sees it: shape and dtype (no device)."""

    def __init__(self, *shape, dtype=np.float32):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.size = int(np.prod(shape, dtype=np.int64))


def test_operators_exist_with_the_reference_defaults_and_refuse_what_it_refuses():
    from rten_amd import lib, ops
    inorm, bn, lsm = ops.InstanceNormalization(), ops.BatchNormalization(), ops.LogSoftmax()
    assert (inorm.epsilon, inorm.act, inorm.max_inputs()) == (None, None, 3)  # epsilon: Option<f32>, 1e-5 when absent (norm.rs:343)
    assert (bn.epsilon, bn.act, bn.max_inputs()) == (1e-5, None, 5)
    assert (lsm.axis, lsm.max_inputs()) == (-1, 1)
    reg = ops.OpRegistry.with_all_ops()
    assert reg.get("InstanceNormalization") is ops.InstanceNormalization and reg.get("LogSoftmax") is ops.LogSoftmax
    assert reg.get("BatchNormalization") is ops.BatchNormalization
    for s in ("rten_hip_instance_norm_f32", "rten_hip_set_instance_norm_path", "rten_hip_batch_norm_f32_act", "rten_hip_log_softmax_f32"):
        assert s in lib.PROTOTYPES and hasattr(lib.load(), s), s
    assert lib.INSTANCE_NORM_RESIDENT_MAX == 32768  # RTEN_HIP_INSTANCE_NORM_RESIDENT_MAX
    header = open(os.path.join(ROOT, "include", "rten_hip.h")).read()
    assert "#define RTEN_HIP_INSTANCE_NORM_RESIDENT_MAX 32768" in header and "#define RTEN_HIP_ABI_VERSION 8" in header

    def refusal(op, inputs):
        with pytest.raises(ops.OpError) as e:
            op.run(None, inputs)
        return e.value.kind, e.value.msg

    x, v3 = _Shape(2, 3, 4, 4), _Shape(3)
    assert refusal(inorm, [_Shape(5), v3, v3]) == ("InvalidValue", "expected input with >= 2 dims")
    assert refusal(inorm, [x, _Shape(4), v3]) == ("InvalidValue", "scale length should match channel count")
    assert refusal(inorm, [x, v3, _Shape(2)]) == ("InvalidValue", "bias length should match channel count")
    assert refusal(inorm, [x, v3])[0] == "MissingInputs"
    assert refusal(inorm, [_Shape(2, 3, 4, dtype=np.int32), v3, v3])[0] == "InputCastFailed"
    assert refusal(bn, [_Shape(), v3, v3, v3, v3]) == ("InvalidValue", "Input must have at least 1 dim")
    for i, nm in enumerate(("scale", "bias", "mean", "var")):
        inputs = [x, v3, v3, v3, v3]
        inputs[1 + i] = _Shape(2)
        assert refusal(bn, inputs) == ("IncompatibleInputShapes", f"{nm}.size(0) != channels")
    assert refusal(bn, [_Shape(7), v3, v3, v3, v3]) == ("IncompatibleInputShapes", "scale.size(0) != channels")  # a 1-D input has one channel
    assert refusal(lsm, [_Shape(2, 3, dtype=np.int32)])[0] == "InputCastFailed"
    assert refusal(ops.LogSoftmax(axis=2), [_Shape(2, 3)]) == ("InvalidValue", "Axis is invalid")


# ---------------------------------------------------------------------------------------------- the loader, through rten_hip_run --parse-only
def _te():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export as te
    return te


def _parse(tmp_path, model_bytes, *flags):
    from tests.test_graph_executor import run_cli
    p = tmp_path / "m.onnx"
    p.write_bytes(model_bytes)
    return run_cli("--parse-only", *flags, str(p))


def _ops_of(stdout):
    line = [l for l in stdout.splitlines() if "canonical form" in l]
    line = line[0].split("nodes:")[1] if line else [l for l in stdout.splitlines() if l.strip().startswith("operators:")][0].split("operators:")[1]
    return set(line.split()[::2])


def _norm_steps(stdout):
    return [l.strip().split()[2] for l in stdout.splitlines() if l.strip().startswith("norm step ")]


@pytest.mark.parametrize("dynamic", [False, True])
def test_exported_generator_loads_its_instance_norms_and_fuses_the_relus(tmp_path, dynamic):
    out = _parse(tmp_path, _te().generator_onnx(dynamic=dynamic))
    assert out.returncode == 0, out.stderr
    assert _ops_of(out.stdout) <= {"Add", "Conv", "ConvTranspose", "InstanceNormalization", "Relu", "Tanh"}, out.stdout  # no Pad node
    steps = _norm_steps(out.stdout)
    assert len(steps) == 7 and steps.count("InstanceNormalization+Relu") == 5 and steps.count("InstanceNormalization") == 2, out.stdout
    unfused = _parse(tmp_path, _te().generator_onnx(dynamic=dynamic), "--no-fuse")
    assert _norm_steps(unfused.stdout) == ["InstanceNormalization"] * 7, unfused.stdout


@pytest.mark.parametrize("dynamic", [False, True])
def test_exported_preact_net_keeps_its_batch_norms_and_fuses_the_activations(tmp_path, dynamic):
    out = _parse(tmp_path, _te().preact_onnx(dynamic=dynamic))
    assert out.returncode == 0, out.stderr
    assert _ops_of(out.stdout) <= {"Add", "BatchNormalization", "Conv", "Flatten", "Gemm", "GlobalAveragePool", "LeakyRelu", "MaxPool", "Relu"}, out.stdout
    assert _norm_steps(out.stdout) == ["BatchNormalization+Relu", "BatchNormalization+LeakyRelu", "BatchNormalization"], out.stdout


@pytest.mark.parametrize("dynamic", [False, True])
def test_exported_recognizer_with_its_log_softmax_head_loads(tmp_path, dynamic):
    te = _te()
    out = _parse(tmp_path, te.recognizer_onnx(te.recognizer_module("gru", log_softmax=True), dynamic=dynamic))
    assert out.returncode == 0, out.stderr
    known = {"Add", "Concat", "ConstantOfShape", "Conv", "Expand", "Gather", "MatMul", "Relu", "Reshape", "Shape", "Slice", "Squeeze", "Transpose", "Unsqueeze", "GRU",
             "LogSoftmax"}
    assert _ops_of(out.stdout) <= known and "LogSoftmax" in _ops_of(out.stdout), out.stdout
    assert [l for l in out.stdout.splitlines() if l.strip().startswith("norm step LogSoftmax")][0].strip().endswith("axis 2"), out.stdout
    assert te.recognizer_onnx(te.recognizer_module("gru")) == te.recognizer_onnx(te.recognizer_module("gru", log_softmax=False))  # the default is unchanged


def _bn_model(attrs, outputs=("y",)):
    from rten_amd import onnx_writer as ow
    v = lambda name, val: ow.tensor(name, np.full(3, val, np.float32))
    nodes = [ow.node("BatchNormalization", ["x", "scale", "bias", "mean", "var"], list(outputs), name="bn_node", **attrs)]
    return ow.model(nodes, [ow.value_info("x", 1, [2, 3, 4, 4])], [ow.value_info("y", 1, [2, 3, 4, 4])], [v("scale", 1.0), v("bias", 0.0), v("mean", 0.0), v("var", 1.0)])


@pytest.mark.parametrize("attrs,outputs,needle", [
    ({"training_mode": 1}, ("y",), "training_mode=1"),
    ({"spatial": 0}, ("y",), "spatial=0"),
    ({}, ("y", "rm"), "running_mean"),
    ({}, ("y", "", "rv"), "running_var"),
])
def test_loader_refuses_training_batch_norm_and_names_the_node(tmp_path, attrs, outputs, needle):
    out = _parse(tmp_path, _bn_model(attrs, outputs))
    assert out.returncode == 1, out.stdout
    assert "bn_node" in out.stderr and "BatchNormalization" in out.stderr and needle in out.stderr, out.stderr


def test_loader_accepts_inference_batch_norm_and_ignores_momentum(tmp_path):
    out = _parse(tmp_path, _bn_model({"momentum": 0.5, "epsilon": 1e-3, "training_mode": 0, "spatial": 1}, ("y", "", "")))
    assert out.returncode == 0, out.stderr
    assert 'norm step BatchNormalization "bn_node": epsilon 0.001' in out.stdout, out.stdout
