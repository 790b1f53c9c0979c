"""RMSNormalization / SimplifiedLayerNormalization, SkipLayerNormalization / SkipSimplifiedLayerNormalization and the two RotaryEmbedding operators without a
GPU: the rules file (tests/decoder_rules.py) against every literal of the reference's tests (tests/golden/decoder_reference.json) within the reference's own
bar, and bit for bit against the oracle's LayerNormalization where the two overlap; both registries, the header's additions with the ABI version unchanged;
the Python operators on a recording context (defaults, the arguments of each launch, every error string of the golden file, refused before anything is
launched); and the builder graphs through the loader's --parse-only checks."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import decoder_rules as R
from tests.reduce_rules import RuleError, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "decoder_reference.json")))
TOL = GOLDEN["tolerance"]


def close(got, want, tol, what):
    """expect_equal_with_tolerance(.., tol, 0.0): absolute."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert float(np.abs(got - want).max(initial=0.0)) <= tol, (what, float(np.abs(got - want).max()))


def arr(v, dtype=F):
    return np.asarray(v, dtype)


# ---------------------------------------------------------------------------------------------- 1. the rules against the reference's literals
@pytest.mark.parametrize("case", GOLDEN["rotary"] + GOLDEN["rotary_batched"], ids=lambda c: c["name"])
def test_rotary_rule_gives_the_reference_s_literals(case):
    ids = None if case["position_ids"] is None else arr(case["position_ids"], I)
    got = R.rotary_embedding(arr(case["input"]), arr(case["cos_cache"]), arr(case["sin_cache"]), ids, case["interleaved"], case["num_heads"], case["rotary_embedding_dim"])
    close(got, case["expected"], TOL["rotary"], case["name"])


def test_contrib_rotary_rule_literals_inference_and_the_offset_form():
    for case in GOLDEN["rotary_contrib"]:
        got = R.rotary_embedding_microsoft(arr(case["input"]), arr(case["position_ids"], I), arr(case["cos_cache"]), arr(case["sin_cache"]), case["interleaved"],
                                           case["num_heads"], case["rotary_embedding_dim"])
        close(got, case["expected"], TOL["rotary"], case["name"])
    c = GOLDEN["rotary_contrib_offset"]
    x, cos, sin = arr(c["input"]), arr(c["cos_cache"]), arr(c["sin_cache"])
    want = R.rotary_embedding_microsoft(x, arr(c["explicit"], I), cos, sin, False, c["num_heads"], c["rotary_embedding_dim"])
    for shape in c["offset_shapes"]:
        got = R.rotary_embedding_microsoft(x, np.full(shape, c["offset"], I), cos, sin, False, c["num_heads"], c["rotary_embedding_dim"])
        close(got, want, TOL["rotary_offset"], f"offset of shape {shape}")
        same_bits(got, want, f"offset of shape {shape}")


def naive_skip_norm(x, skip, gamma, beta, bias, eps, subtract_mean):
    """reference_skip_layer_norm (src/ops/norm/contrib.rs:317-353): the naive float32 formula the reference holds its operator to."""
    last = x.shape[-1]
    total = (x + np.broadcast_to(skip, x.shape)).astype(F)
    total = (total + (bias if bias is not None else np.zeros(last, F))).astype(F)
    rows = total.reshape(-1, last)
    out = np.empty_like(rows)
    for i, row in enumerate(rows):
        mean = F(np.sum(row, dtype=F) / F(last)) if subtract_mean else F(0)
        var = F(np.sum(((row - mean) ** 2).astype(F), dtype=F) / F(last))
        out[i] = ((row - mean) / np.sqrt(F(var + F(eps)))) * gamma + (beta if beta is not None else F(0))
    return out.reshape(x.shape), total


def test_skip_norm_rules_meet_the_reference_s_bar_on_its_shape_table():
    from oracle import ref
    g = GOLDEN["skip_norm"]
    rng = ref.XorShiftRng(g["rng_seed"])
    rand = lambda shape: rng.f32(int(np.prod(shape))).reshape(shape)
    for rms in (False, True):
        for case in g["shape_cases"]:
            last = case["input"][-1]
            x, skip, gamma = rand(case["input"]), rand(case["skip"]), rand([last])
            bias = rand([last]) if case["bias"] else None
            beta = None if rms else rand([last])
            y, total = R.skip_norm(x, skip, gamma, beta, bias, g["epsilon"], rms)
            want, want_total = naive_skip_norm(x, skip, gamma, beta, bias, g["epsilon"], not rms)
            close(y, want, TOL["norm"], f"{case} rms {rms}")
            same_bits(total, want_total, f"{case} rms {rms}: the sum")
    o = g["optional_outputs"]
    for rms in (False, True):
        beta = None if rms else arr(o["beta"])
        y, total = R.skip_norm(arr(o["input"]), arr(o["skip"]), arr(o["gamma"]), beta, arr(o["bias"]), g["epsilon"], rms)
        same_bits(total, arr(o["expected_sum"]), "input_skip_bias_sum")
        close(y, naive_skip_norm(arr(o["input"]), arr(o["skip"]), arr(o["gamma"]), beta, arr(o["bias"]), g["epsilon"], not rms)[0], TOL["norm"], "optional outputs")
    for case in g["errors"]:
        for rms in (False, True):
            with pytest.raises(RuleError) as e:
                R.skip_norm(np.zeros(case["input"], F), np.zeros(case["skip"], F), np.zeros(case["gamma"], F), rms=rms)
            assert (e.value.kind, e.value.msg) == (case["kind"], case["error"])


def test_rms_rule_against_the_naive_formula_and_its_errors():
    rng = np.random.default_rng(3)
    for shape, axis, scale_shape in (((2, 3, 40), -1, (40,)), ((2, 3, 40), -2, (3, 40)), ((5, 130), 1, (130,)), ((4, 7), -1, (1,)), ((4, 7), -1, ())):
        x, scale = rng.standard_normal(shape).astype(F), rng.standard_normal(scale_shape).astype(F)
        got = R.rms_normalization(x, scale, axis, 1e-5)
        cols = int(np.prod(shape[axis:]))
        rows = x.reshape(-1, cols).astype(np.float64)
        want = rows / np.sqrt((rows ** 2).mean(axis=1, keepdims=True) + 1e-5) * np.broadcast_to(scale, shape[axis:]).reshape(-1)
        close(got.reshape(-1, cols), want.astype(F), TOL["norm"], f"{shape} axis {axis}")
    for case in GOLDEN["rms_norm"]["errors"]:
        with pytest.raises(RuleError) as e:
            R.rms_normalization(np.zeros(case["input"], F), np.zeros(case["scale"], F), case["axis"])
        assert (e.value.kind, e.value.msg) == (case["kind"], case["error"])
    # overflow of x * x gives r = 0: zeros, and NaN where x is infinite -- reproduced, not repaired
    x = np.array([[1.0, 1e20, -3.0, 2.0], [1.0, np.inf, -3.0, 2.0]], F)
    got = R.rms_normalization(x, np.ones(4, F))
    assert not got[0].any() and np.isnan(got[1, 1]) and not np.delete(got[1], 1).any()
    # a -0 product: +0 behind the one-element scale's mul_add, -0 behind the per-element multiply
    x = np.array([[-0.0, 1.0, 2.0, 3.0]], F)
    assert not np.signbit(R.rms_normalization(x, np.array([2.0], F))[0, 0]) and np.signbit(R.rms_normalization(x, np.full(4, 2.0, F))[0, 0])


def test_rms_rule_has_the_oracle_layer_norm_s_bits_where_the_two_overlap():
    """A row whose ordered Sum is exactly zero has mean 0, so LayerNormalization's SumSquareSub(mean) is SumSquare and its element map is the RMS one: the
    two must then agree bit for bit (per-element scale without bias: (x - 0) * (g * r); one-element scale: mul_add(x - 0, r, 0))."""
    from oracle import ref
    rng = np.random.default_rng(5)
    for cols in (64, 128, 320):
        x = np.empty((3, cols), F)
        for c0 in range(0, cols, 64):  # accumulators u and u + 1 of every lane cancel exactly: x[16 + l] = -x[l], x[48 + l] = -x[32 + l]
            v = rng.standard_normal((3, 2, 16)).astype(F)
            x[:, c0:c0 + 64] = np.concatenate([v[:, 0], -v[:, 0], v[:, 1], -v[:, 1]], axis=1)
        if cols > 64:  # the chunks must cancel as well: every second chunk is the negative of the one before (320 keeps a last chunk that cancels in itself)
            for c0 in range(64, cols - 63, 128):
                x[:, c0:c0 + 64] = -x[:, c0 - 64:c0]
        gamma = rng.standard_normal(cols).astype(F)
        same_bits(R.rms_normalization(x, gamma, -1, 1e-5), ref.layer_norm(x, gamma, None, eps=1e-5), f"{cols} columns, per-element scale")
        same_bits(R.rms_normalization(x, np.array(1.5, F), -1, 1e-5), ref.layer_norm(x, None, None, gamma_scalar=1.5, eps=1e-5), f"{cols} columns, one-element scale")


# ---------------------------------------------------------------------------------------------- 2. registries, header, bindings
def test_registries_header_and_bindings():
    from rten_amd import lib as L
    from rten_amd import ops
    types = ops.OpRegistry.with_all_ops().op_types()
    for name in ("RMSNormalization", "SimplifiedLayerNormalization", "SkipLayerNormalization", "SkipSimplifiedLayerNormalization", "RotaryEmbedding", "RotaryEmbeddingMicrosoft"):
        assert name in types, name
    assert ops.RotaryEmbeddingMicrosoft().name() == "com.microsoft.RotaryEmbedding" and ops.SkipSimplifiedLayerNormalization(1e-5).name() == "SkipSimplifiedLayerNormalisation"
    d = GOLDEN["rms_norm"]["defaults"]
    assert (ops.RMSNormalization().axis, ops.RMSNormalization().epsilon) == (d["axis"], None) and ops.RMSNormalization().max_inputs() == 2
    assert ops.SkipLayerNormalization(1e-5).max_inputs() == 5 and ops.SkipSimplifiedLayerNormalization(1e-5).max_inputs() == 4
    r = ops.RotaryEmbedding()
    assert (r.interleaved, r.num_heads, r.rotary_embedding_dim, r.max_inputs()) == (False, 0, 0, 4)
    m = ops.RotaryEmbeddingMicrosoft()
    assert (m.interleaved, m.num_heads, m.rotary_embedding_dim, m.max_inputs()) == (False, None, 0, 4)
    with pytest.raises(TypeError):
        ops.SkipLayerNormalization()  # epsilon is required (onnx_registry.rs:1918-1922)
    ops_header = open(os.path.join(ROOT, "include", "rten_hip_ops.hpp")).read()
    for line in ('r.register_op<RMSNormalization>("RMSNormalization");', 'r.register_op<SimplifiedLayerNormalization>("SimplifiedLayerNormalization");',
                 'r.register_op<RotaryEmbedding>("RotaryEmbedding");', 'r.register_op<SkipLayerNormalization>("com.microsoft.SkipLayerNormalization");',
                 'r.register_op<SkipSimplifiedLayerNormalization>("com.microsoft.SkipSimplifiedLayerNormalization");',
                 'r.register_op<RotaryEmbeddingMicrosoft>("com.microsoft.RotaryEmbedding");'):
        assert line in ops_header, line
    header = open(os.path.join(ROOT, "include", "rten_hip.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "rten-hip-sys", "src", "lib.rs")).read()
    assert "#define RTEN_HIP_ABI_VERSION 8\n" in header  # additive: the version stays
    for sym, nargs in (("rten_hip_rms_norm_f32", 8), ("rten_hip_skip_norm_f32", 13), ("rten_hip_rotary_embedding_f32", 24)):
        assert re.search(r"int32_t " + sym + r"\(", header), sym
        assert sym in L.PROTOTYPES and L.PROTOTYPES[sym][0] is C.c_int32 and len(L.PROTOTYPES[sym][1]) == nargs, sym
        assert f"pub fn {sym}(" in bindings, sym
        assert hasattr(L.load(), sym)
    assert (ops.SKIP_NORM_LAYER, ops.SKIP_NORM_RMS) == tuple(int(re.search(rf"#define RTEN_HIP_SKIP_NORM_{k} (\d+)", header).group(1)) for k in ("LAYER", "RMS"))
    assert (ops.ROTARY_POS_NONE, ops.ROTARY_POS_IDS, ops.ROTARY_POS_OFFSET) == tuple(int(re.search(rf"#define RTEN_HIP_ROTARY_POS_{k} (\d+)", header).group(1))
                                                                                     for k in ("NONE", "IDS", "OFFSET"))
    for cite in ("src/ops/norm.rs:419-435,571-608", "src/ops/norm/contrib.rs:22-77", "src/ops/embedding.rs:144-194", "src/ops/embedding/contrib.rs:53-73"):
        assert cite in header, cite


# ---------------------------------------------------------------------------------------------- 3. the Python operators on a recording context
def _recording():
    from rten_amd.recording import RecordingCtx

    class Ctx(RecordingCtx):
        def __init__(self):
            super().__init__()
            self.calls = []

        def call(self, name, *args):
            self.calls.append((name, args))
            super().call(name, *args)

    return Ctx()


def _val(a):
    return a.value if hasattr(a, "value") else a


def _launches(ctx):
    return [(name, [_val(a) for a in args]) for name, args in ctx.calls if not name.startswith("rten_hip_mem") and name not in ("rten_hip_malloc", "rten_hip_free")]


def _refused(op, inputs, kind, msg):
    from rten_amd import ops
    ctx = _recording()
    with pytest.raises(ops.OpError) as e:
        op.run(ctx, inputs(ctx))
    assert _launches(ctx) == []  # refused before anything is launched
    assert (e.value.kind, e.value.msg) == (kind, msg), (e.value.kind, e.value.msg)


def test_python_norm_operators_launch_arguments_and_refusals():
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    ctx = _recording()
    t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
    x, gamma = t(2, 3, 40), t(40)
    y = ops.RMSNormalization().run(ctx, [x, gamma])[0]
    (name, a), = _launches(ctx)
    assert name == "rten_hip_rms_norm_f32" and a[:2] == [6, 40] and a[2:4] == [x.ptr, gamma.ptr] and a[4] == 1.0 and abs(a[5] - 1e-5) < 1e-12 and a[6] == y.ptr and y.shape == x.shape
    ctx.calls.clear()
    ops.SimplifiedLayerNormalization(axis=-2, epsilon=1e-6).run(ctx, [x, t(3, 40)])
    (name, a), = _launches(ctx)
    assert name == "rten_hip_rms_norm_f32" and a[:2] == [2, 120] and abs(a[5] - 1e-6) < 1e-12
    ctx.calls.clear()
    ops.RMSNormalization().run(ctx, [x, np.array([0.5], F)])  # a one-element scale (host value): the scalar form, no gamma pointer
    (name, a), = _launches(ctx)
    assert a[3] is None and a[4] == 0.5
    for case in GOLDEN["rms_norm"]["errors"]:
        _refused(ops.RMSNormalization(axis=case["axis"]), lambda c: [DeviceTensor(c, case["input"], F), DeviceTensor(c, case["scale"], F)], case["kind"], case["error"])
    _refused(ops.RMSNormalization(), lambda c: [DeviceTensor(c, (2, 4), I), DeviceTensor(c, (4,), F)], "InputCastFailed", "expected float32 tensor")

    g = GOLDEN["skip_norm"]
    for case in g["shape_cases"]:
        for rms in (False, True):
            ctx.calls.clear()
            op = ops.SkipSimplifiedLayerNormalization(g["epsilon"]) if rms else ops.SkipLayerNormalization(g["epsilon"])
            last = case["input"][-1]
            xs, skip, gm, extra = t(*case["input"]), t(*case["skip"]), t(last), t(last)
            ins = [xs, skip, gm] + ([extra] if rms and case["bias"] else []) + ([t(last), extra if case["bias"] else None] if not rms else [])
            out = op.run(ctx, ins, outputs=[True, False, False, True])
            (name, a), = _launches(ctx)
            rows = int(np.prod(case["input"][:-1]))
            assert name == "rten_hip_skip_norm_f32" and a[:3] == [1 if rms else 0, rows, last] and a[3:5] == [xs.ptr, skip.ptr] and a[5] == int(np.prod(case["skip"][:-1]))
            assert (a[6] is not None) == case["bias"] and a[7] == gm.ptr and (a[8] is not None) == (not rms)
            assert len(out) == g["optional_outputs"]["n_outputs"] and out[1] is None and out[2] is None and a[10] == out[3].ptr and a[11] == out[0].ptr
            ctx.calls.clear()
            assert len(op.run(ctx, ins)) == 1 and _launches(ctx)[0][1][10] is None  # the sum is written only when it is asked for
    for case in g["errors"]:
        for op in (ops.SkipLayerNormalization(1e-5), ops.SkipSimplifiedLayerNormalization(1e-5)):
            _refused(op, lambda c: [DeviceTensor(c, case["input"], F), DeviceTensor(c, case["skip"], F), DeviceTensor(c, case["gamma"], F)], case["kind"], case["error"])
    _refused(ops.SkipLayerNormalization(1e-5), lambda c: [DeviceTensor(c, (2, 4), F), DeviceTensor(c, (2, 4), F), DeviceTensor(c, (3,), F)],
             "InvalidValue", "`scale` is not broadcastable to normalized axes of input")
    _refused(ops.SkipLayerNormalization(1e-5), lambda c: [DeviceTensor(c, (2, 4), F), DeviceTensor(c, (2, 4), F), DeviceTensor(c, (1, 4), F)],
             "InputCastFailed", "expected tensor with 1 dims")
    _refused(ops.SkipLayerNormalization(1e-5), lambda c: [DeviceTensor(c, (2, 4), F), DeviceTensor(c, (2, 4), F)], "MissingInputs", "")


def test_python_rotary_operators_launch_arguments_and_refusals():
    from rten_amd import einsum as E
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    ctx = _recording()
    t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
    # [B, S, H * D] with caches by (b, s): strides of x and y, broadcast strides of the caches
    x, cos, sin = t(2, 3, 4 * 8), t(1, 3, 4), t(2, 1, 4)
    y = ops.RotaryEmbedding(num_heads=4).run(ctx, [x, cos, sin])[0]
    (name, a), = _launches(ctx)
    assert name == "rten_hip_rotary_embedding_f32" and a[:6] == [2, 3, 4, 8, 8, 0] and a[6:10] == [x.ptr, 96, 32, 8] and a[10:13] == [cos.ptr, 0, 4] and a[13:16] == [sin.ptr, 4, 0]
    assert a[16:19] == [None, ops.ROTARY_POS_NONE, 0] and a[19:] == [y.ptr, 96, 32, 8] and y.shape == x.shape
    # [B, H, S, D] with device ids: the head stride is S * D
    ctx.calls.clear()
    x4, ids, cache = t(2, 4, 3, 8), t(2, 3, dtype=I), t(16, 3)
    ops.RotaryEmbedding(interleaved=True, rotary_embedding_dim=6).run(ctx, [x4, cache, cache, ids])
    (name, a), = _launches(ctx)
    assert a[:6] == [2, 3, 4, 8, 6, 1] and a[7:10] == [96, 8, 24] and a[16:19] == [ids.ptr, ops.ROTARY_POS_IDS, 16] and a[20:] == [96, 8, 24]
    # the contrib form: a one-element device offset is handed to the kernel, nothing is read back; num_heads inferred from the cache
    ctx.calls.clear()
    off, cache4 = t(1, dtype=I), t(16, 4)
    ops.RotaryEmbeddingMicrosoft().run(ctx, [x, off, cache4, cache4])
    assert [n for n, _ in ctx.calls if "d2h" in n] == []
    (name, a), = _launches(ctx)
    assert a[:6] == [2, 3, 4, 8, 8, 0] and a[16:19] == [off.ptr, ops.ROTARY_POS_OFFSET, 16]
    # a q block of a fused projection as a view: read in place through its strides
    ctx.calls.clear()
    qkv = t(2, 3, 96)
    ops.RotaryEmbeddingMicrosoft(num_heads=4).run(ctx, [E.View(qkv, [2, 3, 32], [288, 96, 1]), t(dtype=I), cache4, cache4])
    (name, a), = _launches(ctx)
    assert a[6:10] == [qkv.ptr, 288, 96, 8] and a[20:] == [96, 32, 8]
    # host-known positions are checked on the host, with Gather's message
    ge = GOLDEN["gather_error"]
    _refused(ops.RotaryEmbedding(num_heads=4), lambda c: [DeviceTensor(c, (2, 3, 32), F), DeviceTensor(c, (16, 4), F), DeviceTensor(c, (16, 4), F), np.array([[0, 1, 16], [0, 1, 2]])],
             ge["kind"], ge["error"])
    _refused(ops.RotaryEmbeddingMicrosoft(num_heads=4), lambda c: [DeviceTensor(c, (2, 3, 32), F), np.array([14]), DeviceTensor(c, (16, 4), F), DeviceTensor(c, (16, 4), F)],
             ge["kind"], ge["error"])
    _refused(ops.RotaryEmbeddingMicrosoft(num_heads=4), lambda c: [DeviceTensor(c, (2, 3, 32), F), np.array(-17), DeviceTensor(c, (16, 4), F), DeviceTensor(c, (16, 4), F)],
             ge["kind"], ge["error"])
    for case in GOLDEN["rotary_errors"]:
        if case["op"] == "RotaryEmbedding":
            op = ops.RotaryEmbedding(False, case["num_heads"], case["rotary_embedding_dim"])
            ins = lambda c, case=case: [DeviceTensor(c, case["input_shape"], F), DeviceTensor(c, case["cos_shape"], F), DeviceTensor(c, case["sin_shape"], F)]
        else:
            op = ops.RotaryEmbeddingMicrosoft(False, case["num_heads"], case["rotary_embedding_dim"])
            ins = lambda c, case=case: [DeviceTensor(c, case["input_shape"], F), DeviceTensor(c, case["ids_shape"], I), DeviceTensor(c, case["cos_shape"], F),
                                        DeviceTensor(c, case["sin_shape"], F)]
        _refused(op, ins, case["kind"], case["error"])
        with pytest.raises(RuleError) as e:  # ... and the rules refuse the same cases with the same words
            if case["op"] == "RotaryEmbedding":
                R.rotary_embedding(np.zeros(case["input_shape"], F), np.zeros(case["cos_shape"], F), np.zeros(case["sin_shape"], F), None, False, case["num_heads"],
                                   case["rotary_embedding_dim"])
            else:
                R.rotary_embedding_microsoft(np.zeros(case["input_shape"], F), np.zeros(case["ids_shape"], I), np.zeros(case["cos_shape"], F), np.zeros(case["sin_shape"], F),
                                             False, case["num_heads"], case["rotary_embedding_dim"])
        assert (e.value.kind, e.value.msg) == (case["kind"], case["error"])
    with pytest.raises(RuleError) as e:
        R.gather0(np.zeros((4, 2), F), np.array([[0, 4]]))
    assert (e.value.kind, e.value.msg) == (ge["kind"], ge["error"])


# ---------------------------------------------------------------------------------------------- 4. the builder graphs, through the loader's checks
def _parse_only(tmp_path, name, data, *extra):
    from tests.test_graph_executor import run_cli
    p = tmp_path / name
    p.write_bytes(data)
    return run_cli("--parse-only", *extra, str(p))


def _steps(out):
    return [ln.strip() for ln in out.stdout.splitlines() if ln.strip().startswith("decoder step")]


def test_every_operator_form_parses_and_prints_its_step(tmp_path):
    """Fails on a tree without the operators: its --parse-only prints no `decoder step` line (and its loader refuses the graphs at the first of these nodes:
    "operator SimplifiedLayerNormalization is not available on the HIP backend (no CPU fallback)", "operator domain com.microsoft is not supported")."""
    from rten_amd import onnx_writer as ow
    kinds = {"rms": "RMSNormalization", "rms_two_axes": "RMSNormalization", "rms_one_element_scale": "RMSNormalization", "simplified": "SimplifiedLayerNormalization",
             "skip_layer": "com.microsoft.SkipLayerNormalization", "skip_layer_plain": "com.microsoft.SkipLayerNormalization",
             "skip_simplified": "com.microsoft.SkipSimplifiedLayerNormalization", "skip_simplified_batch_skip": "com.microsoft.SkipSimplifiedLayerNormalization",
             "add_rms": "Add+RMSNormalization", "add_simplified_sole": "Add+SimplifiedLayerNormalization", "rotary": "RotaryEmbedding", "rotary_ids_4d": "RotaryEmbedding",
             "rotary_interleaved_partial": "RotaryEmbedding", "ms_rotary_offset": "com.microsoft.RotaryEmbedding", "ms_rotary_ids": "com.microsoft.RotaryEmbedding"}
    assert set(kinds) == set(ow.NORM_ROTARY_FORMS)
    for form in ow.NORM_ROTARY_FORMS:
        out = _parse_only(tmp_path, form + ".onnx", ow.norm_rotary_graph(form)[0])
        assert out.returncode == 0, out.stdout + out.stderr
        steps = _steps(out)
        assert len(steps) == 1 and steps[0].startswith(f"decoder step {kinds[form]} \""), (form, out.stdout)
    # the Add fusion appears only when fused
    for form, plain in (("add_rms", "RMSNormalization"), ("add_simplified_sole", "SimplifiedLayerNormalization")):
        fused = _steps(_parse_only(tmp_path, form + ".onnx", ow.norm_rotary_graph(form)[0]))
        unfused = _steps(_parse_only(tmp_path, form + ".onnx", ow.norm_rotary_graph(form)[0], "--no-fuse"))
        assert fused == [f'decoder step Add+{plain} "residual" + "norm": one skip launch, epsilon {"1e-06" if form == "add_rms" else "1e-05"}'], fused
        assert unfused == [f'decoder step {plain} "norm": axis -1, epsilon {"1e-06" if form == "add_rms" else "1e-05"}'], unfused
    assert _steps(_parse_only(tmp_path, "s.onnx", ow.norm_rotary_graph("skip_layer")[0])) == [
        'decoder step com.microsoft.SkipLayerNormalization "skip_norm": epsilon 1e-05, bias yes, sum written by the same launch']
    assert _steps(_parse_only(tmp_path, "s.onnx", ow.norm_rotary_graph("skip_layer_plain")[0])) == [
        'decoder step com.microsoft.SkipLayerNormalization "skip_norm": epsilon 1e-05, bias no, sum not read']
    assert _steps(_parse_only(tmp_path, "r.onnx", ow.norm_rotary_graph("rotary_interleaved_partial")[0])) == [
        'decoder step RotaryEmbedding "rope": interleaved 1, num_heads 2, rotary_embedding_dim 6, positions from input 3 (gathered by the kernel)']


def test_decoder_block_graph_parses_fused_and_unfused(tmp_path):
    from rten_amd import onnx_writer as ow
    data, w = ow.decoder_block_graph()
    want = ['decoder step com.microsoft.SkipSimplifiedLayerNormalization "input_norm": epsilon 1e-06, bias no, sum written by the same launch',
            'decoder step com.microsoft.RotaryEmbedding "q_rope": interleaved 0, num_heads 4, rotary_embedding_dim 0, positions from input 1 (ids or a one-element offset, gathered by the kernel)',
            'decoder step com.microsoft.RotaryEmbedding "k_rope": interleaved 0, num_heads 2, rotary_embedding_dim 0, positions from input 1 (ids or a one-element offset, gathered by the kernel)',
            'decoder step com.microsoft.SkipSimplifiedLayerNormalization "post_attention_norm": epsilon 1e-06, bias no, sum written by the same launch']
    for extra in ((), ("--no-fuse",)):
        out = _parse_only(tmp_path, "block.onnx", data, *extra)
        assert out.returncode == 0, out.stdout + out.stderr
        assert _steps(out) == want, out.stdout
        for part in ("SkipSimplifiedLayerNormalization x2", "RotaryEmbedding x2", "MatMul x9", "Concat x2", "Expand x2", "Softmax x1", "Silu x1"):
            assert part in out.stdout, part
    assert sorted(w) == ["cos", "ln1_g", "ln2_g", "sin", "w_down", "w_gate", "w_up", "wk", "wo", "wq", "wv"] and ow.DECODER_BLOCK_OUTPUTS == ["mlp_out", "residual_out", "present_k", "present_v"]


def test_loader_refuses_by_node_name_under_parse_only(tmp_path):
    from rten_amd import onnx_writer as ow
    words = {"stash_type_0": ("RMSNormalization norm:", "stash_type = 0"), "skip_mean_read": ("com.microsoft.SkipLayerNormalization skip_norm:", 'output 1 (mean, "mean") is read'),
             "skip_inv_std_var_output": ("com.microsoft.SkipLayerNormalization skip_norm:", 'output 2 (inv_std_var, "inv_std_var") is read'),
             "skip_no_epsilon": ("com.microsoft.SkipLayerNormalization skip_norm:", "the epsilon attribute is missing"),
             "rms_int_scale": ("RMSNormalization norm:", 'input 1 ("gamma")', "float32 only"), "rotary_int_cache": ("RotaryEmbedding rope:", 'input 1 ("cos3")', "float32 only"),
             "ms_rotary_no_ids": ("com.microsoft.RotaryEmbedding rope:", "position_ids", "required")}
    assert set(words) == set(ow.NORM_ROTARY_BAD)
    for form in ow.NORM_ROTARY_BAD:
        out = _parse_only(tmp_path, form + ".onnx", ow.norm_rotary_graph(form)[0])
        assert out.returncode == 1 and all(w in out.stderr for w in words[form]), (form, out.stderr)
