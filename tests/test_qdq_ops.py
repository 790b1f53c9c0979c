"""QuantizeLinear / DequantizeLinear without a GPU: the rules (tests/qdq_rules.py) against the reference's literal cases, the agreement of the reference's
own code paths inside the contract domain, the host operators' validation, the loader (rten_hip_run --parse-only) and the load-time fold of constant
DequantizeLinear nodes (tests/cpp/qdq_fold_dump.cpp)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import qdq_rules as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "qdq_reference.json")))["cases"]
F = np.float32


def golden_operands(case):
    dt = np.dtype(case["dtype"])
    x = np.array(case["input"], dt)
    scale = np.array(case["scale"], np.float32)
    zp = None if case["zero_point"] is None else np.array(case["zero_point"], dt)
    return x, scale, zp


# ---------------------------------------------------------------------------------------------- 1. the reference's literal cases
@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_rules_reproduce_the_reference_cases(case):
    x, scale, zp = golden_operands(case)
    if "error" in case:
        with pytest.raises(Q.RuleError) as e:
            Q.dequantize_linear(x, scale, zp, case["axis"])
        assert (e.value.kind, e.value.msg) == (case["error"]["kind"], case["error"]["msg"])
        return
    want = np.array(case["expected"], np.float32).reshape(x.shape)
    got = Q.dequantize_linear(x, scale, zp, case["axis"])
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # re-quantising the result gives the input back (quantize.rs:658-670)
    back = Q.quantize_linear(got, scale, zp, case["axis"], dtype=x.dtype)
    assert back.dtype == x.dtype and np.array_equal(back, x)


def test_the_golden_file_holds_every_error_string():
    msgs = {c["error"]["msg"] for c in GOLDEN if "error" in c}
    assert msgs == {"zero_point length does not match size of quantization axis", "scale and zero_point must have same shape",
                    "scale length does not match size of quantization axis", "Blocked dequantization is not supported"}
    assert sum("error" in c for c in GOLDEN) == 5


def test_output_type_rules():
    u8, i8 = np.zeros((), np.uint8), np.zeros((), np.int8)
    assert Q.output_dtype(u8, None) == np.uint8 and Q.output_dtype(i8, None) == np.int8
    assert Q.output_dtype(None, np.uint8) == np.uint8 and Q.output_dtype(None, np.int8) == np.int8
    assert Q.output_dtype(u8, np.uint8) == np.uint8
    for zp, attr in ((None, None), (u8, np.int8), (i8, np.uint8), (np.zeros((), np.int32), None), (None, np.int32)):
        with pytest.raises(Q.RuleError) as e:
            Q.output_dtype(zp, attr)
        assert e.value.kind == "UnsupportedType"


# ---------------------------------------------------------------------------------------------- 2. the reference's forms agree inside the contract domain
def _integer_definition(x, inv, zp, lo, hi):
    """saturate(round_ties_even(x * inv) + zp) with the sum in exact integers: what every form must give where the product is finite."""
    p = (np.asarray(x, F) * F(inv)).astype(F)
    return np.clip(np.rint(p.astype(np.float64)).astype(object) + int(zp), lo, hi).astype(np.int64)


@pytest.mark.parametrize("zp", [0, 1, 128, 255])
def test_u8_forms_agree_on_seeded_inputs(zp):
    rng = np.random.default_rng(100 + zp)
    for n in (1, 63, 64, 65, 200, 4099):
        for scale in (F(0.02), F(1.0), F(3.1e-3), F(7.5)):
            inv = Q.inv_scale_of(scale)
            x = (rng.standard_normal(n) * 300 * scale).astype(F)  # products around +-300: both saturation ends are reached
            x[rng.integers(0, n, max(n // 8, 1))] *= F(1e6)       # ... and far beyond, still below 2^31
            assert np.abs(x * inv).max() < 2.0 ** 31 - 256
            a = Q.quantize_u8_chunked(x, inv, zp)
            assert np.array_equal(a, Q.quantize_scalar(x, inv, zp, np.uint8))
            assert np.array_equal(a, Q.quant_u8_rule(x, inv, zp))
            assert np.array_equal(a, _integer_definition(x, inv, zp, 0, 255))
            assert np.array_equal(a, Q.quantize_linear(x, np.array(scale), np.array(zp, np.uint8)))


def test_pinned_points():
    scale = F(0.25)  # a power of two: x = p * scale is exact, so the products are exactly the ties
    inv = Q.inv_scale_of(scale)
    assert inv == F(4.0)
    ties = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -0.0, 0.0], F)
    x = (ties * scale).astype(F)
    assert np.array_equal((x * inv).astype(F).view(np.uint32), ties.view(np.uint32))
    want = np.array([0, 0, 2, -2, 2, -2, 0, 0])
    for zp in (0, 255, 3):
        exp = np.clip(want + zp, 0, 255)
        for form in (Q.quantize_u8_chunked, Q.quant_u8_rule, lambda a, b, c: Q.quantize_scalar(a, b, c, np.uint8)):
            assert np.array_equal(form(np.tile(x, 9), inv, zp), np.tile(exp, 9)), zp  # 72 elements: a vector chunk and a tail
    for zp in (-128, 127, 0, -5):
        assert np.array_equal(Q.quantize_scalar(x, inv, zp, np.int8), np.clip(want + zp, -128, 127)), zp
    # both saturation ends, one step inside and outside
    for zp in (0, 255, 100):
        p = np.array([-zp - 1, -zp, -zp + 1, 254 - zp, 255 - zp, 256 - zp, 1e9, -1e9], F)
        exp = np.clip(p.astype(np.int64) + zp, 0, 255)
        for form in (Q.quantize_u8_chunked, Q.quant_u8_rule, lambda a, b, c: Q.quantize_scalar(a, b, c, np.uint8)):
            assert np.array_equal(form(np.tile(p, 9), F(1.0), zp), np.tile(exp, 9)), zp
    for zp in (-128, 127, 0):
        p = np.array([-129 - zp, -128 - zp, -127 - zp, 126 - zp, 127 - zp, 128 - zp, 1e9, -1e9], F)
        assert np.array_equal(Q.quantize_scalar(p, F(1.0), zp, np.int8), np.clip(p.astype(np.int64) + zp, -128, 127)), zp
    # a subnormal scale whose reciprocal is finite
    tiny = F(1.1e-38)
    assert 0 < tiny < np.finfo(np.float32).tiny and np.isfinite(Q.inv_scale_of(tiny))
    xs = (np.arange(-70, 70, dtype=np.float32) * tiny).astype(F)
    a = Q.quantize_u8_chunked(xs, Q.inv_scale_of(tiny), 64)
    assert np.array_equal(a, Q.quantize_scalar(xs, Q.inv_scale_of(tiny), 64, np.uint8)) and np.array_equal(a, Q.quant_u8_rule(xs, Q.inv_scale_of(tiny), 64))
    assert np.array_equal(a, _integer_definition(xs, Q.inv_scale_of(tiny), 64, 0, 255)) and len(set(a.tolist())) > 100
    # products just below 2^31 (the largest float32 below it is 2^31 - 128), with every zero point for which round + zp still fits an i32
    edge = np.tile(np.array([2147483520.0, -2147483520.0, 2147483392.0], F), 30)
    for zp in (0, 127):
        for form in (Q.quantize_u8_chunked, Q.quant_u8_rule, lambda a, b, c: Q.quantize_scalar(a, b, c, np.uint8)):
            assert np.array_equal(form(edge, F(1.0), zp), np.tile(np.array([255, 0, 255]), 30))
    for zp in (-128, 127):
        assert np.array_equal(Q.quantize_scalar(edge, F(1.0), zp, np.int8), np.tile(np.array([127, -128, 127]), 30))


def test_outside_the_domain_the_forms_disagree_and_the_documented_rule_is_fixed():
    """NaN, +-inf and products >= 2^31: the vector chunk, its scalar tail and the scalar definition differ (which is why the contract stops there); the
    device follows quant_u8 for per-tensor u8 and the scalar definition elsewhere."""
    x = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9], F)
    assert Q.quant_u8_rule(x, F(1.0), 7).tolist() == [0, 0, 0, 0, 0]
    assert Q.quantize_scalar(x, F(1.0), 7, np.uint8).tolist() == [0, 255, 0, 255, 0]
    assert Q.quantize_scalar(x, F(1.0), 7, np.int8).tolist() == [0, 127, -128, 127, -128]
    vec = Q.quantize_u8_chunked(np.concatenate([np.tile(x, 13)[:64], x[:1]]), F(1.0), 7)  # 64 vector elements + 1 tail element (a NaN)
    assert vec[:5].tolist() == [0, 0, 0, 0, 0] and vec[64] == 7  # the tail's saturating cast turns NaN into 0, then adds the zero point
    assert Q.quantize_linear(x, np.array(1.0, F), np.array(7, np.uint8)).tolist() == [0, 0, 0, 0, 0]
    assert Q.quantize_linear(x.reshape(1, 5), np.ones(5, F), np.full(5, 7, np.uint8), axis=1).tolist() == [[0, 255, 0, 255, 0]]


def test_dequantize_rules():
    big = np.array([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24) - 1, 2 ** 31 - 1, -(2 ** 31)], np.int32)
    got = Q.dequantize_linear(big, np.array(1.0, F))
    assert got.tolist() == [2.0 ** 24, 2.0 ** 24 + 4, -(2.0 ** 24), 2.0 ** 31, -(2.0 ** 31)]  # int -> f32 rounds to nearest even
    wrap = Q.dequantize_linear(np.array([2 ** 31 - 1, -(2 ** 31)], np.int32), np.array(1.0, F), np.array(-1, np.int32))
    assert wrap.tolist() == [-(2.0 ** 31), -(2.0 ** 31)]  # 2^31 - 1 + 1 wraps; -2^31 + 1 rounds back to -2^31
    x = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    s, z = np.array([0.5, 2.0, 0.1], F), np.array([1, 2, 3], np.uint8)
    want = ((x.astype(np.int32) - z.reshape(1, 3, 1).astype(np.int32)).astype(F) * s.reshape(1, 3, 1)).astype(F)
    assert np.array_equal(Q.dequantize_linear(x, s, z, axis=1), want) and np.array_equal(Q.dequantize_linear(x, s, z, axis=-2), want)
    rt = Q.quantize_dequantize(want, s, z, axis=1)
    assert np.array_equal(rt, want)


# ---------------------------------------------------------------------------------------------- 3. host operators on a recording context
class _Shape:
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
    assert reg.get("QuantizeLinear") is ops.QuantizeLinear and reg.get("DequantizeLinear") is ops.DequantizeLinear
    for s in ("rten_hip_quantize_linear_f32", "rten_hip_dequantize_linear_f32", "rten_hip_quantize_dequantize_f32"):
        assert s in lib.PROTOTYPES and hasattr(lib.load(), s), s
    header = open(os.path.join(ROOT, "include", "rten_hip.h")).read()
    for name, value in (("DT_U8", 2), ("DT_I8", 3), ("DT_I32", 1)):
        assert getattr(lib, name) == value and f"#define RTEN_HIP_{name} {value}\n" in header
    assert "#define RTEN_HIP_ABI_VERSION 8" in header
    assert (ops.QuantizeLinear().axis, ops.DequantizeLinear().axis) == (-1, 1)  # the reference's defaults (onnx_registry.rs:1081-1092,1560-1582)


@pytest.mark.parametrize("case", [c for c in GOLDEN if "error" in c], ids=[c["name"] for c in GOLDEN if "error" in c])
def test_operators_refuse_the_reference_cases(case):
    from rten_amd import ops
    x, scale, zp = golden_operands(case)
    shapes = [_Shape(*x.shape, dtype=x.dtype), _Shape(*scale.shape), None if zp is None else _Shape(*zp.shape, dtype=zp.dtype)]
    assert _refusal(ops.DequantizeLinear(axis=case["axis"]), shapes) == (case["error"]["kind"], case["error"]["msg"])
    # QuantizeLinear: the same rules ("quantization" in the blocked message); its per-axis zero-point length check is the one deviation from the reference
    qshapes = [_Shape(*x.shape), shapes[1], shapes[2]]
    want = (case["error"]["kind"], case["error"]["msg"].replace("dequantization", "quantization"))
    assert _refusal(ops.QuantizeLinear(axis=case["axis"], output_dtype=np.uint8), qshapes) == want


def test_operators_refuse_types_and_axes():
    from rten_amd import ops
    x, s = _Shape(2, 3), _Shape()
    assert _refusal(ops.QuantizeLinear(), [x, s])[0] == "UnsupportedType"                                      # neither a zero point nor output_dtype
    assert _refusal(ops.QuantizeLinear(output_dtype=np.int8), [x, s, _Shape(dtype=np.uint8)])[0] == "UnsupportedType"
    assert _refusal(ops.QuantizeLinear(), [x, s, _Shape(dtype=np.int32)])[0] == "UnsupportedType"
    assert _refusal(ops.QuantizeLinear(), [_Shape(2, 3, dtype=np.int32), s, _Shape(dtype=np.uint8)])[0] == "InputCastFailed"
    assert _refusal(ops.QuantizeLinear(), [x])[0] == "MissingInputs"
    assert _refusal(ops.DequantizeLinear(), [x, s])[0] == "UnsupportedType"                                    # float32 data
    assert _refusal(ops.DequantizeLinear(), [_Shape(2, 3, dtype=np.uint8), s, _Shape(dtype=np.int8)])[0] == "InputCastFailed"
    assert _refusal(ops.DequantizeLinear(axis=2), [_Shape(2, 3, dtype=np.int8), _Shape(3)]) == ("InvalidValue", "Axis is invalid")
    assert _refusal(ops.QuantizeLinear(axis=-3), [x, _Shape(3), _Shape(3, dtype=np.int8)]) == ("InvalidValue", "Axis is invalid")
    assert _refusal(ops.QuantizeLinear(axis=1), [x, _Shape(3), _Shape(3, 1, dtype=np.int8)]) == ("InvalidValue", "scale and zero point must have same shape")
    assert _refusal(ops.DequantizeLinear(axis=1), [_Shape(2, 3, dtype=np.int8), _Shape(3), _Shape(3, 1, dtype=np.int8)]) == ("InvalidValue", "scale and zero point must have same rank")


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

    y, log = launches(ops.QuantizeLinear(), [t(2, 3, 4), t(), t(dtype=np.uint8)])
    assert log == ["rten_hip_quantize_linear_f32"] and y.dtype == np.uint8 and y.shape == (2, 3, 4)  # no read-back of scale or zero point
    y, log = launches(ops.QuantizeLinear(axis=1), [t(2, 3, 4), t(3), t(3, dtype=np.int8)])
    assert log == ["rten_hip_quantize_linear_f32"] and y.dtype == np.int8
    y, log = launches(ops.QuantizeLinear(output_dtype=np.int8), [t(5), t(1)])
    assert log == ["rten_hip_quantize_linear_f32"] and y.dtype == np.int8
    for dt in (np.uint8, np.int8, np.int32):
        y, log = launches(ops.DequantizeLinear(axis=0), [t(4, 2, dtype=dt), t(4), t(4, dtype=dt)])
        assert log == ["rten_hip_dequantize_linear_f32"] and y.dtype == np.float32 and y.shape == (4, 2)
    y, log = launches(ops.DequantizeLinear(axis=0), [t(0, dtype=np.uint8), t(0), t(0, dtype=np.uint8)])
    assert log == [] and y.shape == (0,) and y.dtype == np.float32  # empty in, empty out, no launch
    y, log = launches(ops.QuantizeLinear(axis=0), [t(0), t(0), t(0, dtype=np.uint8)])
    assert log == [] and y.shape == (0,) and y.dtype == np.uint8


# ---------------------------------------------------------------------------------------------- 4. the loader, through rten_hip_run --parse-only
def parse_only(tmp_path, data, *flags):
    from tests.test_graph_executor import run_cli
    p = tmp_path / "m.onnx"
    p.write_bytes(data)
    return run_cli("--parse-only", *flags, str(p))


def encoder_qdq():
    from rten_amd import onnx_writer as ow
    from rten_amd.workloads.bert import BertConfig, make_weights
    cfg = BertConfig(hidden=32, heads=2, layers=1, ffn=64, vocab=50, max_pos=16)
    w = make_weights(cfg, 3)
    data, q = ow.bert_encoder_qdq(cfg, w, 8)
    return cfg, w, data, q


def test_small_cnn_qdq_loads(tmp_path):
    from rten_amd import onnx_writer as ow
    data, q = ow.small_cnn_qdq()
    assert q["folded"] == len(q["weight"]) + len(q["bias"]) == 10 and q["pairs"] == 8
    out = parse_only(tmp_path, data)
    assert out.returncode == 0, out.stderr + out.stdout
    assert f"canonical form: {q['folded']} constant DequantizeLinear folded into float32 initializers" in out.stdout
    assert "DequantizeLinear x18" in out.stdout and "QuantizeLinear x8" in out.stdout                       # as written: 8 pairs + 10 constants
    fused = [l for l in out.stdout.splitlines() if "qdq step QuantizeLinear+DequantizeLinear" in l]
    assert len(fused) == q["pairs"] and any('"x.quant" + "x.dequant"' in l for l in fused) and any('"logits.quant" + "logits.dequant"' in l for l in fused)
    assert "qdq step DequantizeLinear" not in out.stdout and "qdq step QuantizeLinear \"" not in out.stdout  # nothing is left on its own
    unfused = parse_only(tmp_path, data, "--no-fuse")
    assert unfused.returncode == 0 and "QuantizeLinear+DequantizeLinear" not in unfused.stdout
    assert unfused.stdout.count("qdq step QuantizeLinear \"") == 8 and unfused.stdout.count("qdq step DequantizeLinear \"") == 8
    # the quantised logits as the graph output: the last pair has no DequantizeLinear
    data8, q8 = ow.small_cnn_qdq(quantized_output=True)
    out8 = parse_only(tmp_path, data8)
    assert out8.returncode == 0 and out8.stdout.count("qdq step QuantizeLinear+DequantizeLinear") == 7 and 'qdq step QuantizeLinear "logits.quant"' in out8.stdout
    assert "output logits.q: u8" in out8.stdout


def test_encoder_qdq_loads(tmp_path):
    cfg, w, data, q = encoder_qdq()
    assert q["folded"] == 6 and q["pairs"] == 4 and q["weight"]["l0.w1"][3] == 1 and q["weight"]["l0.wq"][3] is None
    out = parse_only(tmp_path, data)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "canonical form: 6 constant DequantizeLinear folded into float32 initializers" in out.stdout
    assert out.stdout.count("qdq step QuantizeLinear+DequantizeLinear") == 4 and '"x0.quant" + "x0.dequant"' in out.stdout


def _qdq_model(q_attrs=None, dq_attrs=None, q_inputs=("x", "s", "z"), inits=None):
    from rten_amd import onnx_writer as ow
    nodes = [ow.node("QuantizeLinear", list(q_inputs), ["q"], name="quant_node", **(q_attrs or {})),
             ow.node("DequantizeLinear", ["q", "s", "z"][:len(q_inputs)], ["y"], name="dequant_node", **(dq_attrs or {}))]
    inits = inits if inits is not None else [ow.tensor("s", np.array(0.5, np.float32)), ow.tensor("z", np.array(3, np.uint8))]
    return ow.model(nodes, [ow.value_info("x", ow.FLOAT, [2, 3])], [ow.value_info("y", ow.FLOAT, [2, 3])], inits, opset=21)


@pytest.mark.parametrize("q_attrs, dq_attrs, q_inputs, needle", [
    ({"block_size": 2}, None, ("x", "s", "z"), ("QuantizeLinear quant_node", "block_size")),
    (None, {"block_size": 4}, ("x", "s", "z"), ("DequantizeLinear dequant_node", "block_size")),
    ({"saturate": 0}, None, ("x", "s", "z"), ("QuantizeLinear quant_node", "saturate")),
    ({"precision": 1}, None, ("x", "s", "z"), ("QuantizeLinear quant_node", "precision")),
    (None, {"output_dtype": 10}, ("x", "s", "z"), ("DequantizeLinear dequant_node", "output_dtype")),
    ({"output_dtype": 4}, None, ("x", "s", "z"), ("QuantizeLinear quant_node", "output_dtype")),   # UINT16
    ({"output_dtype": 17}, None, ("x", "s"), ("QuantizeLinear quant_node", "output_dtype")),       # FLOAT8E4M3FN
    (None, None, ("x", "s"), ("QuantizeLinear quant_node", "neither a zero-point input nor output_dtype")),
])
def test_loader_refusals_name_the_node(tmp_path, q_attrs, dq_attrs, q_inputs, needle):
    out = parse_only(tmp_path, _qdq_model(q_attrs, dq_attrs, q_inputs))
    assert out.returncode != 0 and all(n in out.stderr for n in needle), out.stderr + out.stdout


def test_loader_accepts_the_default_attributes_spelled_out(tmp_path):
    out = parse_only(tmp_path, _qdq_model({"block_size": 0, "saturate": 1, "precision": 0, "output_dtype": 2, "axis": 1}, {"block_size": 0, "output_dtype": 0}))
    assert out.returncode == 0 and 'qdq step QuantizeLinear+DequantizeLinear "quant_node" + "dequant_node"' in out.stdout, out.stderr + out.stdout
    out = parse_only(tmp_path, _qdq_model({"output_dtype": 3}, None, ("x", "s")))  # INT8 from output_dtype, no zero point on either node
    assert out.returncode == 0 and "QuantizeLinear+DequantizeLinear" in out.stdout, out.stderr + out.stdout


def test_pairs_that_must_not_fuse(tmp_path):
    from rten_amd import onnx_writer as ow
    s, z = ow.tensor("s", np.array(0.5, np.float32)), ow.tensor("z", np.array(3, np.uint8))
    vi = lambda n, t=ow.FLOAT: ow.value_info(n, t, [2, 3])

    def lines(nodes, outputs, inits):
        out = parse_only(tmp_path, ow.model(nodes, [vi("x")], outputs, inits, opset=21))
        assert out.returncode == 0, out.stderr + out.stdout
        return out.stdout

    q = ow.node("QuantizeLinear", ["x", "s", "z"], ["q"], name="qn")
    dq = lambda scale="s", zp="z", name="dn", out="y", **a: ow.node("DequantizeLinear", ["q", scale, zp], [out], name=name, **a)
    assert "QuantizeLinear+DequantizeLinear" in lines([q, dq()], [vi("y")], [s, z])
    # another scale value / another zero point / two readers / the quantised value is a graph output
    s2, z2 = ow.tensor("s2", np.array(0.25, np.float32)), ow.tensor("z2", np.array(4, np.uint8))
    assert "QuantizeLinear+DequantizeLinear" not in lines([q, dq(scale="s2")], [vi("y")], [s, z, s2])
    assert "QuantizeLinear+DequantizeLinear" not in lines([q, dq(zp="z2")], [vi("y")], [s, z, z2])
    assert "QuantizeLinear+DequantizeLinear" not in lines([q, dq(), dq(name="dn2", out="y2")], [vi("y"), vi("y2")], [s, z])
    assert "QuantizeLinear+DequantizeLinear" not in lines([q, dq()], [vi("y"), vi("q", ow.UINT8)], [s, z])
    # equal values under another name fuse (ort writes one initializer per node); a run-time scale does not
    s_same = ow.tensor("s_copy", np.array(0.5, np.float32))
    assert "QuantizeLinear+DequantizeLinear" in lines([q, dq(scale="s_copy")], [vi("y")], [s, z, s_same])
    rt = [ow.node("Abs", ["x"], ["xs"], name="abs"), ow.node("ReduceMax", ["xs"], ["rs"], name="rmax", keepdims=0),
          ow.node("QuantizeLinear", ["x", "rs", "z"], ["q"], name="qn"), ow.node("DequantizeLinear", ["q", "rs", "z"], ["y"], name="dn")]
    assert "QuantizeLinear+DequantizeLinear" not in lines(rt, [vi("y")], [z])
    # per-axis: the same axis fuses, different axis attributes do not
    sv, zv = ow.tensor("s", np.array([0.5, 0.25, 2.0], np.float32)), ow.tensor("z", np.array([1, 2, 3], np.uint8))
    qa = lambda axis: ow.node("QuantizeLinear", ["x", "s", "z"], ["q"], name="qn", axis=axis)
    assert "QuantizeLinear+DequantizeLinear" in lines([qa(1), dq(axis=1)], [vi("y")], [sv, zv])
    assert "QuantizeLinear+DequantizeLinear" not in lines([qa(-1), dq(axis=1)], [vi("y")], [sv, zv])


# ---------------------------------------------------------------------------------------------- 5. the load-time fold of constant DequantizeLinear
FOLD_BIN = os.path.join(ROOT, "tests", "cpp", "_build", "qdq_fold_dump")


def build_fold_dump():
    from rten_amd import lib as L
    L.load()
    os.makedirs(os.path.dirname(FOLD_BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "qdq_fold_dump.cpp")
    deps = [src] + [os.path.join(ROOT, "include", h) for h in ("rten_hip_graph.hpp", "rten_hip_ops.hpp", "rten_hip.h")]
    if not os.path.exists(FOLD_BIN) or os.path.getmtime(FOLD_BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", FOLD_BIN, "-L" + os.path.join(ROOT, "rten_amd"),
                               "-lrten_hip", "-Wl,-rpath,$ORIGIN/../../../rten_amd", "-Wl,-rpath," + os.path.join(ROOT, "rten_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return FOLD_BIN


def fold(tmp_path, data):
    """-> (exit status, stderr, folded count, {initializer name: array})"""
    p = tmp_path / "fold.onnx"
    p.write_bytes(data)
    out = subprocess.run([build_fold_dump(), str(p)], capture_output=True, text=True, timeout=120)
    inits, folded = {}, None
    types = {1: np.float32, 2: np.uint8, 3: np.int8, 6: np.int32, 7: np.int64}
    for line in out.stdout.splitlines():
        f = line.split(" ")
        if f[0] == "folded":
            folded = int(f[1])
        elif f[0] == "init":
            dims = [int(d) for d in f[3].strip("[]").split(",") if d]
            inits[f[1]] = np.frombuffer(bytes.fromhex(f[4] if len(f) > 4 else ""), types[int(f[2])]).reshape(dims)
    return out.returncode, out.stderr, folded, inits


def test_the_host_fold_gives_the_rules_bits(tmp_path):
    from rten_amd import onnx_writer as ow
    rng = np.random.default_rng(5)
    consts = {
        "w_i8": (rng.integers(-128, 128, (4, 3, 2, 2)).astype(np.int8), rng.uniform(1e-3, 0.1, 4).astype(np.float32), rng.integers(-5, 5, 4).astype(np.int8), 0),
        "a_u8": (rng.integers(0, 256, (3, 5)).astype(np.uint8), np.array(0.0123, np.float32), np.array(131, np.uint8), 1),
        "b_i32": (np.array([2 ** 24 + 1, -(2 ** 24) - 3, 2 ** 31 - 1, -(2 ** 31), 12345, 2 ** 25 + 2], np.int32), rng.uniform(1e-6, 1e-4, 6).astype(np.float32), None, 0),
        "v_u8": (rng.integers(0, 256, (2, 3)).astype(np.uint8), np.array([0.5], np.float32), np.array([10], np.uint8), 0),   # a one-element vector scale: per-tensor
        "c_i8": (rng.integers(-128, 128, (6, 5)).astype(np.int8), rng.uniform(1e-3, 0.1, 5).astype(np.float32), np.zeros(5, np.int8), 1),  # per column
    }
    nodes, inits, outs = [], [], []
    for name, (x, s, z, axis) in consts.items():
        inits += [ow.tensor(name, x), ow.tensor(name + ".s", s)] + ([] if z is None else [ow.tensor(name + ".z", z)])
        nodes.append(ow.node("DequantizeLinear", [name, name + ".s"] + ([] if z is None else [name + ".z"]), [name + ".f"], name=name + ".dq", axis=axis))
        nodes.append(ow.node("Identity", [name + ".f"], [name + ".out"], name=name + ".id"))
        outs.append(ow.value_info(name + ".out", ow.FLOAT, list(x.shape)))
    # a quantised constant that another node still reads stays
    nodes.append(ow.node("Cast", ["a_u8"], ["a_cast"], name="keep", to=ow.FLOAT))
    outs.append(ow.value_info("a_cast", ow.FLOAT, [3, 5]))
    rc, err, folded, got = fold(tmp_path, ow.model(nodes, [], outs, inits, opset=19))
    assert rc == 0 and folded == len(consts), err
    for name, (x, s, z, axis) in consts.items():
        want = Q.dequantize_linear(x, s, z, axis)
        assert got[name + ".f"].dtype == np.float32 and got[name + ".f"].shape == want.shape
        assert np.array_equal(got[name + ".f"].view(np.uint32), want.view(np.uint32)), name
    assert abs(int(consts["b_i32"][0][0])) > 2 ** 24
    # the int8 / int32 initializers nobody reads any more are dropped; the one with a second reader is kept
    assert set(got) == {n + ".f" for n in consts} | {"a_u8"}


def test_the_host_fold_leaves_run_time_operands_alone(tmp_path):
    from rten_amd import onnx_writer as ow
    nodes = [ow.node("DequantizeLinear", ["x", "s", "z"], ["y"], name="dq")]
    rc, err, folded, got = fold(tmp_path, ow.model(nodes, [ow.value_info("x", ow.UINT8, [4])], [ow.value_info("y", ow.FLOAT, [4])],
                                                   [ow.tensor("s", np.array(0.5, np.float32)), ow.tensor("z", np.array(3, np.uint8))]))
    assert rc == 0 and folded == 0 and set(got) == {"s", "z"}, err


@pytest.mark.parametrize("scale, zp, needle", [
    (np.array([0.5, 0.25], np.float32), None, "scale length does not match size of quantization axis"),
    (np.array([0.5, 0.25, 1.0], np.float32), np.array([1, 2], np.int8), "zero_point length does not match size of quantization axis"),
    (np.ones((3, 2), np.float32), None, "Blocked dequantization is not supported"),
    (np.array(0.5, np.float32), np.array([1, 2], np.int8), "scale and zero_point must have same shape"),
])
def test_the_host_fold_names_the_node_it_refuses(tmp_path, scale, zp, needle):
    from rten_amd import onnx_writer as ow
    inits = [ow.tensor("w", np.zeros((3, 2), np.int8)), ow.tensor("s", scale)] + ([] if zp is None else [ow.tensor("z", zp)])
    nodes = [ow.node("DequantizeLinear", ["w", "s"] + ([] if zp is None else ["z"]), ["wf"], name="weight_dq", axis=0), ow.node("Relu", ["wf"], ["y"], name="relu")]
    rc, err, folded, got = fold(tmp_path, ow.model(nodes, [], [ow.value_info("y", ow.FLOAT, [3, 2])], inits))
    assert rc == 1 and "DequantizeLinear weight_dq" in err and needle in err, err


def test_f32_twin_and_resnet50_builders_load(tmp_path):
    """quantize=False writes the same network without a Q/DQ node (the graph a QDQ graph's time is read against); the ResNet-50 builder folds every weight
    and bias and fuses every pair."""
    from rten_amd import onnx_writer as ow
    from rten_amd.workloads import resnet50
    twin, _ = ow.small_cnn_qdq(quantize=False)
    out = parse_only(tmp_path, twin)
    assert out.returncode == 0 and "QuantizeLinear" not in out.stdout and "Conv x4" in out.stdout and "output logits: f32" in out.stdout, out.stderr + out.stdout
    data, q = ow.resnet50_qdq(resnet50.make_weights(), calibration_image=32)
    assert q["folded"] == 2 * 54 and q["pairs"] == 57
    out = parse_only(tmp_path, data)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "canonical form: 108 constant DequantizeLinear folded into float32 initializers" in out.stdout
    assert out.stdout.count("qdq step QuantizeLinear+DequantizeLinear") == 57 and "qdq step DequantizeLinear" not in out.stdout
