"""GRU / LSTM without a GPU: the numpy restatement (tests/rnn_rules.py) against the reference's own PyTorch fixtures, the bound on the
one deliberate divergence (tanh of the cell state), the host operators' validation, and what the ONNX loader accepts and refuses."""
import json
import os
import sys

import numpy as np
import pytest

from tests import rnn_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "rnn_pytorch.json")  # the reference's pytorch-ref-tests/rnn.json

CASES = ["lstm_forwards", "lstm_initial", "lstm_bidirectional", "gru_forwards", "gru_initial", "gru_bidirectional"]


def _tensor(v):
    shape, data = v
    return np.asarray(data, np.float32).reshape(shape)


def read_case(name):
    """read_pytorch_ref_test (src/ops/rnn.rs:922-1011): batch dim inserted, PyTorch's gate order turned into the reference's."""
    case = json.load(open(FIXTURE))[name]
    lstm = name.startswith("lstm")
    order = ("ifco", "iofc") if lstm else ("ruh", "urh")
    p = case["params"]
    bidi = "weight_ih_l0_reverse" in p
    rd = lambda key: R.reorder_gates(_tensor(p[key]), order[0], order[1], 0)
    sfx = ["", "_reverse"] if bidi else [""]
    out = {
        "lstm": lstm,
        "direction": "bidirectional" if bidi else "forward",
        "x": _tensor(case["input"])[:, None, :],
        "w": np.stack([rd("weight_ih_l0" + s) for s in sfx]),
        "r": np.stack([rd("weight_hh_l0" + s) for s in sfx]),
        "b": np.stack([np.concatenate([rd("bias_ih_l0" + s), rd("bias_hh_l0" + s)]) for s in sfx]),
        "h0": _tensor(case["initial_hidden"])[:, None, :] if "initial_hidden" in case else None,
        "c0": _tensor(case["initial_cell"])[:, None, :] if "initial_cell" in case else None,
    }
    e = _tensor(case["output"])
    out["expected"] = (e.reshape(e.shape[0], 2, e.shape[1] // 2) if bidi else e[:, None, :])[:, :, None, :]
    return out


def run_rules(c, **kw):
    if c["lstm"]:
        return R.lstm(c["x"], c["w"], c["r"], c["b"], c["h0"], c["c0"], c["direction"], **kw)
    return R.gru(c["x"], c["w"], c["r"], c["b"], c["h0"], c["direction"])


def test_fixture_is_the_six_reference_cases():
    assert sorted(k for k in json.load(open(FIXTURE)) if not k.startswith("__")) == sorted(CASES)
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_pytorch_fixtures_at_the_reference_bar(name):
    """expect_equal's defaults (rten-tensor/src/test_util.rs): |a - b| <= atol 1e-8 + rtol 1e-5 * |b|."""
    c = read_case(name)
    y = run_rules(c)[0]
    assert y.shape == c["expected"].shape
    err = np.abs(y.astype(np.float64) - c["expected"])
    bound = 1e-8 + 1e-5 * np.abs(c["expected"].astype(np.float64))
    print(name, "largest |diff|", err.max(), "largest diff / bound", (err / bound).max())
    assert (err <= bound).all()


def test_cell_tanh_divergence_is_within_the_margin_of_libm_tanh():
    """h = o * tanh(c): the reference calls f32::tanh (libm), the backend the vecmath tanh.  Largest deviation from a float64 evaluation over
    the three LSTM fixtures -- restatement (vecmath tanh): 5.57e-08, the same with np.tanh on float32 in that spot: 4.79e-08; the first
    must stay within 4x the second (the margin of the graph-fuzz tests: deviations scatter by about a factor of two between seeds)."""
    dev_vm = dev_libm = 0.0
    for name in CASES[:3]:
        c = read_case(name)
        y64 = R.lstm_f64(c["x"], c["w"], c["r"], c["b"], c["h0"], c["c0"], c["direction"])[0]
        dev_vm = max(dev_vm, np.abs(run_rules(c)[0] - y64).max())
        dev_libm = max(dev_libm, np.abs(run_rules(c, cell_tanh=lambda v: np.tanh(v.astype(np.float32)))[0] - y64).max())
    print(f"deviation from float64: vecmath tanh {dev_vm:.3e}, libm tanh {dev_libm:.3e}")
    assert dev_libm > 0
    assert dev_vm <= 4 * dev_libm


@pytest.mark.parametrize("lstm", [False, True])
@pytest.mark.parametrize("with_bias,with_init", [(False, False), (True, False), (False, True), (True, True)])
def test_last_hidden_state_is_the_sequence_end_of_each_direction(lstm, with_bias, with_init):
    """The reference's random-input test (rnn.rs test_rnn_ops_with_random_input): seq 5, batch 2, features 2, hidden 3, bidirectional."""
    from oracle import ref
    rng = ref.XorShiftRng(1234)
    seq, batch, feat, hid, G = 5, 2, 2, 3, 4 if lstm else 3
    mk = lambda *s: (rng.f32(int(np.prod(s))).reshape(s) - 0.5).astype(np.float32)
    x, w, r = mk(seq, batch, feat), mk(2, G * hid, feat), mk(2, G * hid, hid)
    b = mk(2, 2 * G * hid) if with_bias else None
    h0 = mk(2, batch, hid) if with_init else None
    c0 = mk(2, batch, hid) if with_init else None
    out = R.lstm(x, w, r, b, h0, c0, "bidirectional") if lstm else R.gru(x, w, r, b, h0, "bidirectional")
    y, yh = out[0], out[1]
    assert y.shape == (seq, 2, batch, hid) and yh.shape == (2, batch, hid)
    assert np.array_equal(yh[0], y[-1, 0]) and np.array_equal(yh[1], y[0, 1])
    assert np.isfinite(y).all() and np.abs(y).max() > 0


class _Shape:
    """An operand as the validation sees it: shape and dtype (no device)."""

    def __init__(self, *shape, dtype=np.float32):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)


def test_operators_exist_with_the_reference_defaults_and_refuse_what_it_refuses():
    from rten_amd import lib, ops
    g, l = ops.GRU(), ops.LSTM()
    assert (g.direction, g.linear_before_reset, g.max_inputs()) == ("forward", False, 6)  # onnx_registry.rs:1220: unwrap_or(false)
    assert (l.direction, l.max_inputs()) == ("forward", 7)
    reg = ops.OpRegistry.with_all_ops()
    assert reg.get("GRU") is ops.GRU and reg.get("LSTM") is ops.LSTM
    for s in ("rten_hip_gru_f32", "rten_hip_lstm_f32", "rten_hip_set_rnn_path"):
        assert s in lib.PROTOTYPES and hasattr(lib.load(), s), s
    x, w3, r3, w4, r4 = _Shape(5, 2, 2), _Shape(1, 9, 2), _Shape(1, 9, 3), _Shape(1, 12, 2), _Shape(1, 12, 3)

    def refusal(op, inputs):
        with pytest.raises(ops.OpError) as e:
            op.run(None, inputs)
        return e.value.kind, e.value.msg

    assert refusal(ops.GRU(), [x, w3, r3]) == ("UnsupportedValue", "`linear_before_reset=0` is not supported")
    assert refusal(ops.LSTM(), [x, _Shape(1, 10, 2), r4]) == ("InvalidValue", "weights dim 1 must be 4 * hidden_size")
    assert refusal(ops.LSTM(), [x, w4, r4, _Shape(1, 20)]) == ("InvalidValue", "bias dim 1 must be 8 * hidden_size")
    assert refusal(ops.GRU(linear_before_reset=True), [_Shape(5, 2), w3, r3]) == ("InvalidValue", "input must have 3 dims (seq, batch, input)")
    assert refusal(ops.LSTM(), [x, _Shape(12, 2), r4]) == ("InvalidValue", "weights must have 3 dims (dir, hidden x 4, input)")
    assert refusal(ops.GRU(linear_before_reset=True), [x, w3])[0] == "MissingInputs"


# ---------------------------------------------------------------------------------------------- the loader, through rten_hip_run --parse-only
RECOGNIZERS = [("gru", True, 1, True), ("lstm", True, 2, True), ("gru", False, 2, False), ("lstm", False, 1, False)]  # kind, bidirectional, layers, dynamic axes


def recognizer_bytes(kind, bidirectional, layers, dynamic, seed=0):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export as te
    return te.recognizer_onnx(kind=kind, bidirectional=bidirectional, layers=layers, seed=seed, dynamic=dynamic)


def _parse(tmp_path, model_bytes):
    from tests.test_graph_executor import run_cli
    p = tmp_path / "m.onnx"
    p.write_bytes(model_bytes)
    return run_cli("--parse-only", str(p))


@pytest.mark.parametrize("kind,bidirectional,layers,dynamic", RECOGNIZERS)
def test_exported_recognizers_hold_only_known_operators_and_load_their_recurrent_nodes(tmp_path, kind, bidirectional, layers, dynamic):
    """What PyTorch's exporter writes around nn.GRU / nn.LSTM is in the executor already; the recurrent nodes pass the loader's attribute
    checks (linear_before_reset=1, empty sequence_lens, default activations) and show as steps."""
    out = _parse(tmp_path, recognizer_bytes(kind, bidirectional, layers, dynamic))
    assert out.returncode == 0, out.stderr
    op = kind.upper()
    steps = [l for l in out.stdout.splitlines() if l.strip().startswith("recurrent step " + op)]
    assert len(steps) == layers, out.stdout
    assert all(("bidirectional" if bidirectional else "forward") in l and "hidden_size 20" in l for l in steps)
    canon = [l for l in out.stdout.splitlines() if "canonical form" in l][0].split("nodes:")[1].split()[::2]
    known = {"Add", "Concat", "ConstantOfShape", "Conv", "Expand", "Gather", "MatMul", "Relu", "Reshape", "Shape", "Slice", "Squeeze", "Transpose", "Unsqueeze", op}
    assert set(canon) <= known, canon


def _rnn_model(op, attrs, extra_inputs=(), n_inputs=None):
    from rten_amd import onnx_writer as ow
    G, hid, feat = (4 if op == "LSTM" else 3), 3, 2
    rng = np.random.default_rng(0)
    inits = [ow.tensor("W", rng.standard_normal((1, G * hid, feat)).astype(np.float32)), ow.tensor("R", rng.standard_normal((1, G * hid, hid)).astype(np.float32))]
    inputs = ["x", "W", "R"] + list(extra_inputs)
    for name, arr in (("lens", np.array([5, 5], np.int32)), ("P", np.zeros((1, 3 * hid), np.float32))):
        if name in inputs:
            inits.append(ow.tensor(name, arr))
    base = {"hidden_size": hid}
    if op == "GRU":
        base["linear_before_reset"] = 1
    base.update(attrs)
    nodes = [ow.node(op, inputs, ["y", "y_h"], name="rnn_node", **base)]
    return ow.model(nodes, [ow.value_info("x", 1, [5, 2, feat])], [ow.value_info("y", 1, [5, 1, 2, hid])], inits)


@pytest.mark.parametrize("op,attrs,extra,needle", [
    ("GRU", {"linear_before_reset": 0}, (), "`linear_before_reset=0` is not supported"),
    ("GRU", {"clip": 1.0}, (), "clip"),
    ("LSTM", {"clip": 1.0}, (), "clip"),
    ("GRU", {"layout": 1}, (), "layout"),
    ("LSTM", {"layout": 1}, (), "layout"),
    ("GRU", {"activations": ["Relu", "Tanh"]}, (), "activations"),
    ("LSTM", {"activations": ["Relu", "Tanh", "Tanh"]}, (), "activations"),
    ("LSTM", {"input_forget": 1}, (), "input_forget"),
    ("GRU", {}, ("", "lens"), "sequence_lens"),
    ("LSTM", {}, ("", "lens"), "sequence_lens"),
    ("LSTM", {}, ("", "", "", "", "P"), "peephole"),
])
def test_loader_refuses_what_the_reference_refuses_and_names_the_node(tmp_path, op, attrs, extra, needle):
    out = _parse(tmp_path, _rnn_model(op, attrs, extra))
    assert out.returncode == 1, out.stdout
    assert "rnn_node" in out.stderr and op in out.stderr and needle in out.stderr, out.stderr


def test_loader_accepts_the_default_activations_spelled_out(tmp_path):
    out = _parse(tmp_path, _rnn_model("LSTM", {"activations": ["Sigmoid", "Tanh", "Tanh"], "direction": "forward"}))
    assert out.returncode == 0 and 'recurrent step LSTM "rnn_node": forward, hidden_size 3' in out.stdout, out.stderr
