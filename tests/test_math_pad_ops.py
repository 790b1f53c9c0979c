"""Pad, Pow, the unary math operators, PRelu and the variadic Min / Max / Sum / Mean without a GPU: the expected values (tests/math_rules.py) against
the reference's own test literals and numpy's pad, the bound on the deliberate divergence from the host's libm (Log, Pow, Softplus), the host operators'
validation and launch sequences on a recording context, the host-value evaluator (a g++ program), and what the ONNX loader accepts and refuses
(through rten_hip_run --parse-only)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import math_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "math_pad_reference.json")))
F = np.float32
_SPECIAL = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "-0.0": -0.0}


def _arr(v, shape=None, dtype=np.float32):
    a = np.array([_SPECIAL.get(e, e) if isinstance(e, str) else e for e in v], dtype)
    return a.reshape(shape) if shape is not None else a


def _raises(fn, error):
    with pytest.raises(R.RuleError) as e:
        fn()
    assert [e.value.kind, e.value.msg] == error


# ---------------------------------------------------------------------------------------------- 1. the rules against the reference's literals
@pytest.mark.parametrize("case", GOLDEN["pad"], ids=lambda c: c["cite"].split(" ", 1)[0].split("/")[-1])
def test_pad_rules_reproduce_the_reference_literals(case):
    dt = np.dtype(case.get("dtype", "float32"))
    x = _arr(case["input"], case["shape"], dt)
    run = lambda: R.pad(x, case["pads"], case["mode"])
    if "error" in case:
        return _raises(run, case["error"])
    y = run()
    assert y.dtype == dt and list(y.shape) == case["expected_shape"]
    assert np.array_equal(y.ravel(), _arr(case["expected"], None, dt))  # a Pad moves values: the literals are reproduced exactly


def test_pad_rules_refuse_an_axes_input():
    _raises(lambda: R.pad(np.zeros((2, 2), F), [0, 0, 0, 0], axes=[0]), ["UnsupportedValue", "Pad operator does not yet support `axes` input"])


@pytest.mark.parametrize("case", GOLDEN["unary"], ids=lambda c: c["op"])
def test_unary_rules_reproduce_the_reference_literals(case):
    dt = np.dtype(case.get("dtype", "float32"))
    y = R.UNARY[case["op"]](_arr(case["input"], None, dt))
    want = _arr(case["expected"], None, dt)
    assert y.dtype == dt and R.same_bits(y, want), (y, want)


@pytest.mark.parametrize("case", GOLDEN["prelu"], ids=lambda c: "error" if "error" in c else "values")
def test_prelu_rules_reproduce_the_reference_literals(case):
    run = lambda: R.prelu(_arr(case["x"], case["x_shape"]), _arr(case["slope"], case["slope_shape"]))
    if "error" in case:
        return _raises(run, case["error"])
    assert R.same_bits(run(), _arr(case["expected"]))


@pytest.mark.parametrize("case", GOLDEN["pow"], ids=lambda c: c["cite"].split(" ", 1)[1][:24])
def test_pow_rules_reproduce_the_reference_literals(case):
    base, e = _arr(case["base"]), _arr(case["exponent"], case["exponent_shape"])
    y = R.pow_(base, e)
    if case.get("expected_powf"):
        libm = C.CDLL("libm.so.6")
        libm.powf.restype, libm.powf.argtypes = C.c_float, [C.c_float, C.c_float]
        want = np.array([libm.powf(float(b), float(e)) for b in base], np.float32)
        assert R.ulp_distance(y, want).max() <= 1
    else:
        assert R.same_bits(y, _arr(case["expected"]))


@pytest.mark.parametrize("case", GOLDEN["variadic"], ids=lambda c: c["cite"].split(" ", 1)[1][:32])
def test_variadic_rules_reproduce_the_reference_literals(case):
    fn = {"Max": R.vmax, "Min": R.vmin, "Sum": R.vsum, "Mean": R.mean}[case["op"]]
    inputs = [_arr(i["data"], i["shape"]) for i in case["inputs"]]
    if "error" in case:
        return _raises(lambda: fn(*inputs), case["error"])
    y = fn(*inputs)
    assert list(y.shape) == case["expected_shape"] and R.same_bits(y.ravel(), _arr(case["expected"]))


def test_min_max_keep_the_left_operand_on_a_tie_and_let_either_nan_win():
    pz, nz, nan = F(0.0), F(-0.0), F(np.nan)
    bits = lambda v: int(np.asarray(v, np.float32).view(np.uint32))
    assert bits(R.max2(pz, nz)) == bits(pz) and bits(R.max2(nz, pz)) == bits(nz)
    assert bits(R.min2(pz, nz)) == bits(pz) and bits(R.min2(nz, pz)) == bits(nz)
    for f in (R.min2, R.max2):
        assert np.isnan(f(nan, F(1))) and np.isnan(f(F(1), nan))
    assert bits(R.sign(pz)) == bits(F(1)) and bits(R.sign(nz)) == bits(F(-1)) and np.isnan(R.sign(nan))
    assert bits(R.round_(F(-0.4))) == bits(nz) and R.round_(F(2.5)) == 2 and R.round_(F(3.5)) == 4
    i32 = np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max, -7, 0], np.int32)
    assert R.neg(i32).tolist() == [-2 ** 31, -(2 ** 31 - 1), 7, 0] and R.abs_(i32).tolist() == [-2 ** 31, 2 ** 31 - 1, 7, 0]
    assert R.sign(i32).tolist() == [-1, 1, -1, 0]
    assert R.vsum(i32, np.array([-1, 1, 0, 0], np.int32)).tolist() == [2 ** 31 - 1, -2 ** 31, -7, 0]  # wraps
    assert float(R.mean(F(1), F(1), F(2))) == float(F(4) / F(3))  # divided, not multiplied by the rounded reciprocal


@pytest.mark.parametrize("mode,np_mode", [("reflect", "reflect"), ("edge", "edge"), ("wrap", "wrap"), ("constant", "constant")])
def test_pad_rules_agree_with_numpy_where_both_are_defined(mode, np_mode):
    rng = np.random.default_rng(11)
    for h, w in ((1, 4), (3, 4), (5, 7), (2, 33)):
        x = rng.standard_normal((2, 3, h, w)).astype(np.float32)
        limit = lambda n: n - 1 if mode == "reflect" else n + 2  # numpy's reflect repeats differently from pad == len on; the reference's formula is its own
        for _ in range(6):
            t, b = (int(rng.integers(0, limit(h) + 1)) for _ in range(2))
            l, r = (int(rng.integers(0, limit(w) + 1)) for _ in range(2))
            got = R.pad(x, [0, 0, t, l, 0, 0, b, r], mode, value=F(1.5))
            kw = {"constant_values": F(1.5)} if mode == "constant" else {}
            want = np.pad(x, ((0, 0), (0, 0), (t, b), (l, r)), mode=np_mode, **kw)
            assert np.array_equal(got, want), (mode, h, w, t, l, b, r)


def test_reflect_with_a_pad_of_at_least_the_axis_length_is_the_formula_taken_literally():
    """rem_euclid of the reflected coordinate: for len 3, begin pad 5 the coordinates 0..4 read 5, 4, 3, 2, 1 mod 3."""
    assert R.src_index("reflect", np.arange(11), 3, 5).tolist() == [2, 1, 0, 2, 1, 0, 1, 2, 1, 0, 2]
    assert R.src_index("reflect", np.arange(3), 1, 1).tolist() == [0, 0, 0]
    assert R.src_index("wrap", np.arange(7), 2, 3).tolist() == [1, 0, 1, 0, 1, 0, 1]
    assert R.src_index("edge", np.arange(7), 2, 3).tolist() == [0, 0, 0, 0, 1, 1, 1]


# ---------------------------------------------------------------------------------------------- 2. the rules against the host's libm
def libm_inputs():
    """The seeded inputs of the GPU tests for the operators defined through float64 (tests/test_gpu_math_pad.py imports this)."""
    rng = np.random.default_rng(2024)
    n = 4099
    with np.errstate(all="ignore"):
        log_x = np.exp(rng.uniform(-80, 80, n)).astype(np.float32)
        pow_b = np.exp(rng.uniform(-5, 5, n)).astype(np.float32)
    pow_e = rng.uniform(-6, 6, n).astype(np.float32)
    sp_x = rng.uniform(-100, 95, n).astype(np.float32)
    return log_x, pow_b, pow_e, sp_x


def test_rules_are_within_one_ulp_of_the_hosts_libm_with_equal_specials():
    libm = C.CDLL("libm.so.6")
    for name, nargs in (("logf", 1), ("powf", 2), ("expf", 1), ("log1pf", 1)):
        getattr(libm, name).restype, getattr(libm, name).argtypes = C.c_float, [C.c_float] * nargs
    logf = lambda x: np.array([libm.logf(float(v)) for v in x], np.float32)
    powf = lambda b, e: np.array([libm.powf(float(u), float(v)) for u, v in zip(b, e)], np.float32)
    softplusf = lambda x: np.array([libm.log1pf(libm.expf(float(v))) for v in x], np.float32)
    log_x, pow_b, pow_e, sp_x = libm_inputs()
    for what, got, want in (("Log", R.log(log_x), logf(log_x)), ("Pow", R.pow_(pow_b, pow_e), powf(pow_b, pow_e)), ("Softplus", R.softplus(sp_x), softplusf(sp_x))):
        d = R.ulp_distance(got, want)
        print(f"{what}: {int((d > 0).sum())} of {d.size} differ from libm, largest distance {int(d.max())} ulp")
        assert d.max() <= 1, what
        assert (np.isinf(got) == np.isinf(want)).all(), what
    nan, inf = np.nan, np.inf
    x = np.array([0.0, -0.0, inf, 1.0, nan, -1.0, -inf], np.float32)
    assert R.same_bits(R.log(x), logf(x))
    xs = np.array([0.0, -0.0, inf, -inf, 1.0, nan, 88.7, 88.73, -104.0], np.float32)
    assert R.same_bits(R.softplus(xs), softplusf(xs))
    base = np.array([-2, -0.0, 0.0, 0.5, 1, 2, inf, nan, -inf], np.float32)
    expo = np.array([-inf, -1, -0.5, 0, 0.5, 2, 3, inf, nan, 1, -3], np.float32)
    b, e = (a.ravel() for a in np.meshgrid(base, expo, indexing="ij"))
    assert R.same_bits(R.pow_(b, e), powf(b, e))


# ---------------------------------------------------------------------------------------------- 3. host operators on a recording context
class _Shape:
    """An operand as the validation sees it: shape and dtype (no device)."""

    def __init__(self, *shape, dtype=np.float32):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.size = int(np.prod(shape, dtype=np.int64))


def _refusal(op, inputs):
    from rten_amd import ops
    with pytest.raises(ops.OpError) as e:
        op.run(None, inputs)
    return e.value.kind, e.value.msg


def test_operators_are_registered_and_bound():
    from rten_amd import lib, ops
    reg = ops.OpRegistry.with_all_ops()
    for n in ("Neg", "Abs", "Sign", "Floor", "Ceil", "Round", "Sqrt", "Reciprocal", "Exp", "Log", "Softplus", "Pow", "PRelu", "Min", "Max", "Sum", "Mean", "Pad"):
        assert reg.get(n) is getattr(ops, n), n
    for s in ("rten_hip_unary_f32", "rten_hip_pad_b32"):
        assert s in lib.PROTOTYPES and hasattr(lib.load(), s), s
    header = open(os.path.join(ROOT, "include", "rten_hip.h")).read()
    for name, value in (("UNARY_NEG", 0), ("UNARY_SOFTPLUS", 10), ("UNARY_EXP", 8), ("EW_INEG", 15), ("EW_IMAX", 19), ("EW_IADD", 11), ("PAD_WRAP", 3), ("PAD_CONSTANT", 0)):
        assert getattr(lib, name) == value and f"#define RTEN_HIP_{name} {value}\n" in header, name
    assert "#define RTEN_HIP_ABI_VERSION 8" in header
    assert (ops.Pad().mode, ops.Pad().max_inputs(), ops.Pow().max_inputs(), ops.Max().max_inputs()) == ("constant", 4, 2, None)


def test_operators_refuse_what_the_reference_refuses():
    from rten_amd import ops
    x = _Shape(2, 3, 4, 5)
    pads = lambda *p: np.array(p, np.int32)
    assert _refusal(ops.Pad(), [x, pads(1)]) == ("InvalidValue", "padding length should be 2 * input dims")
    assert _refusal(ops.Pad(), [x, pads(0, 0, -3, 0, 0, 0, -2, 0)]) == ("InvalidValue", "Negative pads remove more elements than axis contains")
    assert _refusal(ops.Pad("reflect"), [x, pads(0, 1, 0, 0, 0, 0, 0, 0)]) == ("UnsupportedValue", "Pad only supports non-constant padding of last 2 dims")
    assert _refusal(ops.Pad("edge"), [_Shape(3, 0), pads(0, 2, 0, 0)]) == ("InvalidValue", "Padded dimension for non-constant padding is empty")
    assert _refusal(ops.Pad(), [x, pads(0, 0, 0, 0, 0, 0, 0, 0), None, pads(0)]) == ("UnsupportedValue", "Pad operator does not yet support `axes` input")
    assert _refusal(ops.Pad(), [x, pads(0, 0, 0, 0, 0, 0, 0, 1), np.array(1, np.int32)])[0] == "InputCastFailed"
    assert _refusal(ops.Pad(), [x, pads(0, 0, 0, 0, 0, 0, 0, 1), np.array([1, 2], np.float32)])[0] == "InputCastFailed"
    assert _refusal(ops.Pad(), [x])[0] == "MissingInputs"
    with pytest.raises(ops.OpError):
        ops.Pad("mirror")
    assert _refusal(ops.PRelu(), [_Shape(5), _Shape(2, 1)]) == ("IncompatibleInputShapes", "Slope is not broadcastable to input shape")
    assert _refusal(ops.Max(), [_Shape(3), _Shape(2, 2)]) == ("IncompatibleInputShapes", "Cannot broadcast inputs")
    assert _refusal(ops.Min(), [_Shape(3), _Shape(3, dtype=np.int32)])[0] == "InputCastFailed"
    assert _refusal(ops.Mean(), [_Shape(3, dtype=np.int32)])[0] == "InputCastFailed"  # Mean is float32 only
    assert _refusal(ops.Max(), [])[0] == "MissingInputs"
    for e_dt in (np.float32, np.int32):
        kind, msg = _refusal(ops.Pow(), [_Shape(3, dtype=np.int32), _Shape(dtype=e_dt)])
        assert kind == "UnsupportedValue" and "Pow" in msg and "int32" in msg
    assert _refusal(ops.Pow(), [_Shape(3), _Shape(dtype=np.int32)]) == ("UnsupportedValue", "Unsupported base and exponent type combination")
    assert _refusal(ops.Sqrt(), [_Shape(3, dtype=np.int32)])[0] == "InputCastFailed"
    assert _refusal(ops.Neg(), [_Shape(3, dtype=np.uint8)])[0] == "UnsupportedType"


def test_launch_sequences_on_a_recording_context():
    from rten_amd import ops
    from rten_amd.recording import RecordingCtx
    from rten_amd.tensor import DeviceTensor
    ctx = RecordingCtx()
    t = lambda *shape, dtype=np.float32: DeviceTensor(ctx, shape, dtype)

    def launches(op, inputs):
        del ctx.log[:]
        out = op.run(ctx, inputs)
        return out[0], [l for l in ctx.log if l != "rten_hip_malloc"]

    y, log = launches(ops.Max(), [t(2, 1, 4), t(3, 1), t(4)])
    assert log == ["rten_hip_binary_broadcast_f32"] * 2 and y.shape == (2, 3, 4)  # a left fold: two launches
    y, log = launches(ops.Max(), [t(2, 3)])
    assert log == ["rten_hip_memcpy_d2d"] and y.shape == (2, 3)  # one input is a copy
    y, log = launches(ops.Min(), [t(2, 3, dtype=np.int32), t(3, dtype=np.int32)])
    assert log == ["rten_hip_elementwise_nd"] and y.dtype == np.int32
    y, log = launches(ops.Mean(), [t(2, 3), t(3), t(2, 1)])
    assert log == ["rten_hip_binary_broadcast_f32", "rten_hip_binary_broadcast_f32", "rten_hip_memcpy_h2d", "rten_hip_div_f32"] and y.shape == (2, 3)
    y, log = launches(ops.Pow(), [t(2, 3), t()])
    assert log == ["rten_hip_binary_broadcast_f32"]
    y, log = launches(ops.Neg(), [t(7, dtype=np.int32)])
    assert log == ["rten_hip_elementwise_nd"] and y.dtype == np.int32
    y, log = launches(ops.Log(), [t(7)])
    assert log == ["rten_hip_unary_f32"]
    y, log = launches(ops.Pad("reflect"), [t(2, 3, 4, 5), np.array([0, 0, 1, 2, 0, 0, 3, 4], np.int32)])
    assert log == ["rten_hip_pad_b32"] and y.shape == (2, 3, 8, 11)  # one launch per Pad
    y, log = launches(ops.Pad(), [t(2, 5), [0, -2, 1, -3]])
    assert log == [] and y.shape == (3, 0)  # a zero-sized output launches nothing
    y, log = launches(ops.Pad(), [t(2, 5, dtype=np.int32), [0, -1, 0, 1], np.array(7, np.int32)])
    assert log == ["rten_hip_pad_b32"] and y.shape == (2, 5) and y.dtype == np.int32


# ---------------------------------------------------------------------------------------------- 4. the host-value evaluator (a g++ program)
HOSTOPS_BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_math_hostops")


def build_hostops_binary():
    from rten_amd import lib as L
    L.load()
    os.makedirs(os.path.dirname(HOSTOPS_BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_math_hostops.cpp")
    deps = [src] + [os.path.join(ROOT, "include", h) for h in ("rten_hip_graph.hpp", "rten_hip_ops.hpp", "rten_hip.h")]
    if not os.path.exists(HOSTOPS_BIN) or os.path.getmtime(HOSTOPS_BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", HOSTOPS_BIN, "-L" + os.path.join(ROOT, "rten_amd"),
                               "-lrten_hip", "-Wl,-rpath,$ORIGIN/../../../rten_amd", "-Wl,-rpath," + os.path.join(ROOT, "rten_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return HOSTOPS_BIN


def test_host_evaluation_of_math_operators_and_constant_pad():
    out = subprocess.run([build_hostops_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------- 5. the loader, through rten_hip_run --parse-only
def _te():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export as te
    return te


def _parse(tmp_path, model_bytes, *flags):
    from tests.test_graph_executor import run_cli
    p = tmp_path / "m.onnx"
    p.write_bytes(model_bytes)
    return run_cli("--parse-only", *flags, str(p))


def _steps(stdout, prefix):
    return [l.strip() for l in stdout.splitlines() if l.strip().startswith(prefix)]


def _ops_of(stdout):
    line = [l for l in stdout.splitlines() if "canonical form" in l]
    line = line[0].split("nodes:")[1] if line else [l for l in stdout.splitlines() if l.strip().startswith("operators:")][0].split("operators:")[1]
    return set(line.split()[::2])


@pytest.mark.parametrize("dynamic", [False, True])
def test_exported_reflect_generator_loads_its_pads_and_prelus(tmp_path, dynamic):
    out = _parse(tmp_path, _te().reflect_generator_onnx(dynamic=dynamic))
    assert out.returncode == 0, out.stderr
    assert _ops_of(out.stdout) == {"Add", "Conv", "InstanceNormalization", "PRelu", "Pad", "Tanh"}, out.stdout
    pads = _steps(out.stdout, "pad step Pad")
    modes = [p.split("mode ")[1].split(",")[0] for p in pads]
    assert modes.count("reflect") == 5 and modes.count("edge") == 1 and modes.count("constant") == 1, out.stdout  # the file really holds Pad nodes with mode=reflect
    assert len(_steps(out.stdout, "math step PRelu")) == 3, out.stdout


def test_exported_gpt2_mlp_keeps_its_pow_node(tmp_path):
    out = _parse(tmp_path, _te().gpt2_mlp_onnx())
    assert out.returncode == 0, out.stderr
    assert {"Pow", "Tanh", "LayerNormalization", "MatMul"} <= _ops_of(out.stdout), out.stdout  # (the LayerNorm's own Pow / Sqrt are part of the fused pattern)
    assert len(_steps(out.stdout, "math step Pow")) == 1, out.stdout


def test_exported_box_decoder_loads_its_math_nodes(tmp_path):
    out = _parse(tmp_path, _te().box_decode_onnx())
    assert out.returncode == 0, out.stderr
    assert {"Exp", "Min", "Max", "Sqrt", "Reciprocal", "Neg", "Abs"} <= _ops_of(out.stdout), out.stdout
    kinds = [s.split()[2] for s in _steps(out.stdout, "math step")]
    assert sorted(kinds) == sorted(["Exp", "Max", "Max", "Min", "Min", "Abs", "Sqrt", "Reciprocal", "Abs", "Neg"]), out.stdout


def test_dynamic_upsample_graph_holds_floor_on_shape_values_and_an_input_form_pad(tmp_path):
    out = _parse(tmp_path, _te().dynamic_upsample_onnx())
    assert out.returncode == 0, out.stderr
    assert {"Shape", "Cast", "Mul", "Floor", "Concat", "Resize", "Pad"} <= _ops_of(out.stdout), out.stdout
    assert _steps(out.stdout, "math step Floor") == ['math step Floor "floor_hw": host-evaluated on host values, device otherwise'], out.stdout
    assert _steps(out.stdout, "pad step Pad") == ['pad step Pad "pad_up": mode constant, pads from input 1 (a host value at run time)'], out.stdout


def _pad_model(mode=None, inputs=("x", "pads"), pads_initializer=True, attrs=None):
    from rten_amd import onnx_writer as ow
    inits = [ow.tensor("pads", np.array([0, 0, 1, 1, 0, 0, 1, 1], np.int64))] if pads_initializer else []
    inits.append(ow.tensor("axes", np.array([2, 3], np.int64)))
    graph_inputs = [ow.value_info("x", 1, [2, 3, 4, 4])] + ([] if pads_initializer else [ow.value_info("pads", 7, [8])])
    kw = dict(attrs or {})
    if mode is not None:
        kw["mode"] = mode
    return ow.model([ow.node("Pad", list(inputs), ["y"], name="pad_node", **kw)], graph_inputs, [ow.value_info("y", 1, [2, 3, 6, 6])], inits)


@pytest.mark.parametrize("model_args,needle", [
    (dict(mode="mirror"), 'mode "mirror"'),
    (dict(mode="reflect", inputs=("x", "pads", "", "axes")), "does not yet support `axes` input"),
    (dict(inputs=("x",)), "the pads input is missing"),
    (dict(pads_initializer=False), "device data at run time"),
])
def test_loader_refuses_pad_forms_and_names_the_node(tmp_path, model_args, needle):
    out = _parse(tmp_path, _pad_model(**model_args))
    assert out.returncode == 1, out.stdout
    assert "pad_node" in out.stderr and "Pad" in out.stderr and needle in out.stderr, out.stderr


def test_loader_accepts_both_pad_forms(tmp_path):
    out = _parse(tmp_path, _pad_model(mode="wrap"))
    assert out.returncode == 0 and 'pad step Pad "pad_node": mode wrap, pads from input 1' in out.stdout, out.stdout + out.stderr
    out = _parse(tmp_path, _pad_model(inputs=("x",), attrs={"pads": [0, 0, 1, 1, 0, 0, 1, 1], "value": 1.5}))  # before opset 11
    assert out.returncode == 0 and 'pad step Pad "pad_node": mode constant, pads from the pads attribute' in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("base", ["initializer", "graph input"])
def test_loader_refuses_pow_with_an_int32_base_and_names_the_node(tmp_path, base):
    from rten_amd import onnx_writer as ow
    inits = [ow.tensor("e", np.array(2.0, np.float32))] + ([ow.tensor("b", np.arange(6, dtype=np.int32))] if base == "initializer" else [])
    graph_inputs = [ow.value_info("x", 1, [6])] + ([] if base == "initializer" else [ow.value_info("b", 6, [6])])
    nodes = [ow.node("Pow", ["b", "e"], ["p"], name="pow_node"), ow.node("Cast", ["p"], ["pf"], name="cast", to=1), ow.node("Add", ["x", "pf"], ["y"], name="add")]
    out = _parse(tmp_path, ow.model(nodes, graph_inputs, [ow.value_info("y", 1, [6])], inits))
    assert out.returncode == 1, out.stdout
    assert "pow_node" in out.stderr and "Pow" in out.stderr and "int32 base" in out.stderr, out.stderr
