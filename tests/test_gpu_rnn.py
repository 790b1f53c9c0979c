"""GRU / LSTM on the device, bit-identical to the numpy restatement of the reference (tests/rnn_rules.py): the C ABI on both paths (the
per-step composed path and the time-persistent fused kernel), the Python host operators, and PyTorch-exported recognisers through the resident
executor (the C++ host operators) node by node, fused, captured into a hipGraph and as replicas."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref
from rten_amd import lib as L
from rten_amd import ops
from rten_amd.tensor import DeviceTensor
from tests import rnn_rules as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTION_CODE = {"forward": L.RNN_FORWARD, "reverse": L.RNN_REVERSE, "bidirectional": L.RNN_BIDIRECTIONAL}


def _cases(lstm):
    """About 24 cases per operator.  hidden: 3 is below an MFMA tile, 20 puts gate boundaries inside one, 64 is whole tiles, 260 crosses the 256-deep
    block of the recurrent product (beyond the fused kernel: composed only); input 257 crosses the block of the input projection; batch 17 is a ragged
    second batch tile; with batch 1, seq 4 / 5 is the switch between the one-row order and the blocked one.  Every direction, B / initial_h /
    initial_c present and absent, every non-empty subset of the outputs."""
    hid, inp, bat, sq = [3, 16, 20, 64, 260], [2, 32, 257], [1, 2, 17], [1, 4, 5, 9]
    n_out = 3 if lstm else 2
    masks = list(range(1, 1 << n_out))
    out = []
    for i in range(20):
        out.append(dict(hidden=hid[i % 5], input=inp[(i + i // 5) % 3], batch=bat[(i + i // 3) % 3], seq=sq[(i + i // 4) % 4], direction=R.DIRECTIONS[i % 3],
                        bias=bool(i & 1), h0=bool(i & 2), c0=bool(i & 4) and lstm, mask=masks[(i + i // 7) % len(masks)]))
    full = masks[-1]
    out += [dict(hidden=20, input=32, batch=1, seq=4, direction="bidirectional", bias=True, h0=True, c0=lstm, mask=full),
            dict(hidden=20, input=32, batch=1, seq=5, direction="bidirectional", bias=True, h0=True, c0=lstm, mask=full),
            dict(hidden=64, input=257, batch=17, seq=9, direction="bidirectional", bias=True, h0=False, c0=False, mask=full),
            dict(hidden=256, input=32, batch=17, seq=5, direction="reverse", bias=True, h0=True, c0=lstm, mask=full),  # the largest size the fused kernel covers
            dict(hidden=260, input=2, batch=2, seq=5, direction="forward", bias=False, h0=False, c0=False, mask=1)]
    return out


def _id(c):
    return f"h{c['hidden']}-i{c['input']}-b{c['batch']}-s{c['seq']}-{c['direction'][:3]}-B{int(c['bias'])}h{int(c['h0'])}c{int(c['c0'])}-o{c['mask']}"


def covered(c):
    """What rten_hip.h states for the fused kernel."""
    return c["hidden"] <= L.RNN_FUSED_MAX_HIDDEN and not (c["batch"] == 1 and c["seq"] < R.PREPACK_MIN_SEQ_LEN)


def make(lstm, c, seed):
    rng = np.random.default_rng(seed)
    G, dirs, H = (4 if lstm else 3), (2 if c["direction"] == "bidirectional" else 1), c["hidden"]
    u = lambda *s, k=1.0: ((rng.random(s, dtype=np.float32) - np.float32(0.5)) * np.float32(2 * k)).astype(np.float32)
    kw, kr = 1.0 / np.sqrt(c["input"]), 1.0 / np.sqrt(H)
    t = dict(x=u(c["seq"], c["batch"], c["input"]), w=u(dirs, G * H, c["input"], k=kw), r=u(dirs, G * H, H, k=kr),
             b=u(dirs, 2 * G * H, k=0.5) if c["bias"] else None, h0=u(dirs, c["batch"], H) if c["h0"] else None,
             c0=u(dirs, c["batch"], H) if c["c0"] else None)
    want = R.lstm(t["x"], t["w"], t["r"], t["b"], t["h0"], t["c0"], c["direction"]) if lstm else R.gru(t["x"], t["w"], t["r"], t["b"], t["h0"], c["direction"])
    return t, want


def bits_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = got.view(np.int32) == np.ascontiguousarray(want).view(np.int32)
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} values differ, first at {tuple(np.argwhere(~same)[0])}: {got[tuple(np.argwhere(~same)[0])]!r} vs {want[tuple(np.argwhere(~same)[0])]!r}"


def run_abi(ctx, lstm, t, c, path, x_dev=None, x_strides=(0, 0)):
    """One call of rten_hip_gru_f32 / rten_hip_lstm_f32 under rten_hip_set_rnn_path(path); outputs outside the mask are NULL."""
    seq, batch, n_in = t["x"].shape
    dirs, H = t["w"].shape[0], c["hidden"]
    dev = {k: (DeviceTensor.from_numpy(ctx, v) if v is not None else None) for k, v in t.items()}
    if x_dev is not None:
        dev["x"] = x_dev
    shapes = [(seq, dirs, batch, H), (dirs, batch, H), (dirs, batch, H)][:3 if lstm else 2]
    outs = [DeviceTensor(ctx, s, np.float32) if c["mask"] >> i & 1 else None for i, s in enumerate(shapes)]
    for o in outs:
        if o is not None:
            o.upload(np.full(o.shape, np.nan, np.float32))  # every element must be written
    geo = (seq, batch, n_in, H, DIRECTION_CODE[c["direction"]])
    vp = lambda v: None if v is None else v.vp
    ctx.call("rten_hip_set_rnn_path", path)
    try:
        if lstm:
            ctx.call("rten_hip_lstm_f32", *geo, x_strides[0], x_strides[1], dev["x"].vp, dev["w"].vp, dev["r"].vp, vp(dev["b"]), vp(dev["h0"]), vp(dev["c0"]), *[vp(o) for o in outs])
        else:
            ctx.call("rten_hip_gru_f32", *geo, 1, x_strides[0], x_strides[1], dev["x"].vp, dev["w"].vp, dev["r"].vp, vp(dev["b"]), vp(dev["h0"]), *[vp(o) for o in outs])
    finally:
        ctx.call("rten_hip_set_rnn_path", L.RNN_PATH_AUTO)
    return [None if o is None else o.numpy() for o in outs]


def check(got, want, c, what):
    for i, name in enumerate(("Y", "Y_h", "Y_c")[:len(want)]):
        if c["mask"] >> i & 1:
            bits_equal(got[i], want[i], f"{what} {name}")
        else:
            assert got[i] is None


@pytest.mark.parametrize("lstm", [False, True], ids=["gru", "lstm"])
@pytest.mark.parametrize("idx", range(25))
def test_c_abi_and_python_operator_give_the_reference_bits_on_both_paths(ctx, lstm, idx):
    c = _cases(lstm)[idx]
    t, want = make(lstm, c, 100 * idx + lstm)
    composed = run_abi(ctx, lstm, t, c, L.RNN_PATH_COMPOSED)
    check(composed, want, c, _id(c) + " composed")
    if covered(c):
        fused = run_abi(ctx, lstm, t, c, L.RNN_PATH_FUSED)
        check(fused, want, c, _id(c) + " fused")
        for a, b in zip(composed, fused):  # the cross-check: two implementations, one set of bits
            assert (a is None and b is None) or np.array_equal(a.view(np.int32), b.view(np.int32))
    else:
        with pytest.raises(L.HipError) as e:
            run_abi(ctx, lstm, t, c, L.RNN_PATH_FUSED)
        assert e.value.code == L.ERR_UNSUPPORTED
    check(run_abi(ctx, lstm, t, c, L.RNN_PATH_AUTO), want, c, _id(c) + " auto")
    # the Python host layer (rten_amd.ops): same entry points behind the operator interface
    direction = c["direction"]
    op = ops.LSTM(direction, c["hidden"]) if lstm else ops.GRU(direction, c["hidden"], linear_before_reset=True)
    dv = lambda v: None if v is None else DeviceTensor.from_numpy(ctx, v)
    inputs = [dv(t["x"]), dv(t["w"]), dv(t["r"]), dv(t["b"]), None, dv(t["h0"])] + ([dv(t["c0"])] if lstm else [])
    outs = op.run(ctx, inputs, outputs=[bool(c["mask"] >> i & 1) for i in range(len(want))])
    check([None if o is None else o.numpy() for o in outs], want, c, _id(c) + " ops")


def test_case_list_reaches_every_edge_on_both_paths():
    for lstm in (False, True):
        cs = _cases(lstm)
        assert len(cs) == 25
        for key, values in (("hidden", [3, 16, 20, 64, 260]), ("input", [2, 32, 257]), ("batch", [1, 2, 17]), ("seq", [1, 4, 5, 9]), ("direction", list(R.DIRECTIONS)),
                            ("bias", [False, True]), ("h0", [False, True]), ("mask", list(range(1, 8 if lstm else 4)))):
            assert {c[key] for c in cs} >= set(values), key
            fusable = [v for v in values if not (key == "hidden" and v > L.RNN_FUSED_MAX_HIDDEN)]
            assert {c[key] for c in cs if covered(c)} >= set(fusable), (key, "on the fused path")
        assert any(c["batch"] == 1 and c["seq"] == 4 for c in cs) and any(c["batch"] == 1 and c["seq"] == 5 for c in cs)


def _kernels_of(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        fn()
        ctx.sync()
        return {e["kernel"] for e in ctx.profile_report()}
    finally:
        ctx.profile(False)
        ctx.profile_reset()


@pytest.mark.parametrize("lstm", [False, True], ids=["gru", "lstm"])
def test_auto_takes_the_composed_path_just_past_the_coverage_limit_and_fused_refuses_it(ctx, lstm):
    name = "lstm" if lstm else "gru"
    past = dict(hidden=L.RNN_FUSED_MAX_HIDDEN + 1, input=2, batch=2, seq=5, direction="forward", bias=True, h0=False, c0=False, mask=1)
    t, want = make(lstm, past, 7)
    kernels = _kernels_of(ctx, lambda: check(run_abi(ctx, lstm, t, past, L.RNN_PATH_AUTO), want, past, "past the limit, auto"))
    assert f"{name}_gate_kernel" in kernels and f"{name}_fused_kernel" not in kernels, kernels
    with pytest.raises(L.HipError) as e:
        run_abi(ctx, lstm, t, past, L.RNN_PATH_FUSED)
    assert e.value.code == L.ERR_UNSUPPORTED and "fused kernel does not cover" in e.value.msg
    op = ops.LSTM("forward", past["hidden"]) if lstm else ops.GRU("forward", past["hidden"], linear_before_reset=True)
    ctx.call("rten_hip_set_rnn_path", L.RNN_PATH_FUSED)
    try:
        with pytest.raises(ops.OpError) as oe:
            op.run(ctx, [DeviceTensor.from_numpy(ctx, t[k]) for k in ("x", "w", "r")])
        assert oe.value.kind == "UnsupportedValue"
    finally:
        ctx.call("rten_hip_set_rnn_path", L.RNN_PATH_AUTO)
    # forcing a path is forcing it: the fused kernel where it is asked for, the gate kernel where that is
    inside = dict(past, hidden=L.RNN_FUSED_MAX_HIDDEN)
    t2, want2 = make(lstm, inside, 8)
    assert f"{name}_fused_kernel" in _kernels_of(ctx, lambda: check(run_abi(ctx, lstm, t2, inside, L.RNN_PATH_FUSED), want2, inside, "at the limit, fused"))
    assert f"{name}_gate_kernel" in _kernels_of(ctx, lambda: run_abi(ctx, lstm, t2, inside, L.RNN_PATH_COMPOSED))


def test_rnn_path_is_part_of_the_tuning_snapshot(ctx):
    state = (C.c_int32 * 8)()
    ctx.call("rten_hip_set_rnn_path", L.RNN_PATH_COMPOSED)
    try:
        ctx.call("rten_hip_tuning_save", state)
        ctx.call("rten_hip_set_rnn_path", L.RNN_PATH_FUSED)
        ctx.call("rten_hip_tuning_restore", state)
        c = dict(hidden=16, input=2, batch=2, seq=5, direction="forward", bias=False, h0=False, c0=False, mask=1)
        t, _ = make(False, c, 3)
        dev = [DeviceTensor.from_numpy(ctx, t[k]) for k in ("x", "w", "r")]
        y = DeviceTensor(ctx, (5, 1, 2, 16), np.float32)
        kernels = _kernels_of(ctx, lambda: ctx.call("rten_hip_gru_f32", 5, 2, 2, 16, 0, 1, 0, 0, dev[0].vp, dev[1].vp, dev[2].vp, None, None, y.vp, None))
        assert "gru_gate_kernel" in kernels and "gru_fused_kernel" not in kernels, kernels
        with pytest.raises(L.HipError):
            ctx.call("rten_hip_set_rnn_path", 3)
    finally:
        ctx.call("rten_hip_set_rnn_path", L.RNN_PATH_AUTO)


@pytest.mark.parametrize("lstm", [False, True], ids=["gru", "lstm"])
@pytest.mark.parametrize("path", [L.RNN_PATH_COMPOSED, L.RNN_PATH_FUSED], ids=["composed", "fused"])
def test_x_is_read_through_its_strides(ctx, lstm, path):
    """X as the exporter's Transpose leaves it: stored [batch, seq, input], read as [seq, batch, input] through element strides -- no copy."""
    c = dict(hidden=20, input=32, batch=17, seq=5, direction="bidirectional", bias=True, h0=True, c0=lstm, mask=7 if lstm else 3)
    t, want = make(lstm, c, 11)
    stored = DeviceTensor.from_numpy(ctx, np.ascontiguousarray(t["x"].transpose(1, 0, 2)))
    got = run_abi(ctx, lstm, t, c, path, x_dev=stored, x_strides=(c["input"], c["seq"] * c["input"]))
    check(got, want, c, "strided X")


# ---------------------------------------------------------------------------------------------- exported recognisers through the resident executor
RECOGNIZERS = [("gru", True, 1, True), ("lstm", True, 2, True), ("gru", False, 2, False), ("lstm", False, 1, False)]  # kind, bidirectional, layers, dynamic axes
_models = {}


def recognizer(kind, bidirectional, layers, dynamic):
    key = (kind, bidirectional, layers, dynamic)
    if key not in _models:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import torch_export as te
        module = te.recognizer_module(kind, bidirectional, layers, seed=len(_models))
        _models[key] = (module, te.recognizer_onnx(module, dynamic=dynamic))
    return _models[key]


def expected_output(module, kind, bidirectional, layers, x):
    """The recogniser composed from the oracle's operators and the recurrent restatement, one graph node at a time."""
    p = {k: v.detach().numpy() for k, v in module.state_dict().items()}
    f = ref.relu(ref.conv2d_f32(x, p["conv.weight"], p["conv.bias"], pads=(1, 1, 1, 1)))
    seq = np.ascontiguousarray(f.transpose(3, 0, 1, 2)).reshape(f.shape[3], f.shape[0], -1)
    order = ("ifco", "iofc") if kind == "lstm" else ("ruh", "urh")
    rd = lambda key: R.reorder_gates(p[key], order[0], order[1], 0)
    for layer in range(layers):
        sfx = [f"_l{layer}", f"_l{layer}_reverse"] if bidirectional else [f"_l{layer}"]
        w = np.stack([rd("rnn.weight_ih" + s) for s in sfx])
        r = np.stack([rd("rnn.weight_hh" + s) for s in sfx])
        b = np.stack([np.concatenate([rd("rnn.bias_ih" + s), rd("rnn.bias_hh" + s)]) for s in sfx])
        direction = "bidirectional" if bidirectional else "forward"
        y = (R.lstm(seq, w, r, b, None, None, direction) if kind == "lstm" else R.gru(seq, w, r, b, None, direction))[0]
        seq = np.ascontiguousarray(y.transpose(0, 2, 1, 3)).reshape(y.shape[0], y.shape[2], -1)
    out = ref.matmul_f32(seq, np.ascontiguousarray(p["head.weight"].T))
    return ref.add(out, p["head.bias"]).reshape(out.shape)


def run_recognizer(tmp_path, data, x, *flags):
    from tests.test_graph_executor import run_cli
    model, xin, yout = tmp_path / "m.onnx", tmp_path / "x.bin", tmp_path / "y.bin"
    model.write_bytes(data)
    xin.write_bytes(np.ascontiguousarray(x, np.float32).tobytes())
    out = run_cli(*flags, "-s", f"batch={x.shape[0]}", "-s", f"width={x.shape[3]}", "--input", f"x={xin}", "--dump", f"y={yout}", str(model))
    assert out.returncode == 0, out.stderr + out.stdout
    return np.fromfile(yout, np.float32), out.stdout


@pytest.mark.parametrize("kind,bidirectional,layers,dynamic", RECOGNIZERS)
def test_exported_recognizers_node_by_node_fused_and_captured(tmp_path, kind, bidirectional, layers, dynamic):
    import torch
    module, data = recognizer(kind, bidirectional, layers, dynamic)
    for batch, width in [(2, 12)] + ([(3, 7)] if dynamic else []):
        x = (np.random.default_rng(batch * 100 + width).random((batch, 1, 8, width), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
        want = expected_output(module, kind, bidirectional, layers, x)
        runs = [run_recognizer(tmp_path, data, x, *flags) for flags in (("--no-fuse",), (), ("--graph", "-n", "3"))]
        assert "Captured the plan into a hipGraph" in runs[2][1]
        for (got, _), mode in zip(runs, ("--no-fuse", "fused", "--graph -n 3")):
            bits_equal(got.reshape(want.shape), want, f"{kind} recogniser {batch}x{width} {mode}")
        with torch.no_grad():
            t = module(torch.from_numpy(x)).numpy()
        diff = np.abs(runs[1][0].reshape(t.shape) - t).max()
        print(f"{kind} bidirectional={bidirectional} layers={layers} {batch}x{width}: max |device - torch| = {diff:.3e}")
        assert diff <= 1e-4  # the bar tests/test_shape_arithmetic.py holds exported graphs to against torch's CPU forward


def test_loading_through_the_executor_names_the_refused_node(tmp_path):
    from tests.test_graph_executor import run_cli
    from tests.test_rnn_ops import _rnn_model
    p = tmp_path / "bad.onnx"
    p.write_bytes(_rnn_model("GRU", {"clip": 1.0}))
    out = run_cli(str(p))
    assert out.returncode == 1 and "rnn_node" in out.stderr and "clip" in out.stderr, out.stderr


def test_replicas_of_one_model_keep_their_own_recurrent_workspace(ctx):
    """rten_hip_model_clone on a second context: the same weights, different inputs, run side by side -- each gets its own expected bits.  The model ABI
    hands outputs over as dim-0 batch slices, so this recogniser ends in a permute to [batch, width, classes]."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export as te
    module = te.recognizer_module("gru", True, 1, seed=9, batch_first=True)
    data = te.recognizer_onnx(module)
    rng = np.random.default_rng(5)
    xs = [(rng.random((2, 1, 8, 12), dtype=np.float32) - np.float32(0.5)).astype(np.float32) for _ in range(2)]
    wants = [np.ascontiguousarray(expected_output(module, "gru", True, 1, x).transpose(1, 0, 2)) for x in xs]
    ctx2 = L.Context(0)
    m = L.Model(ctx, data, None, 1)
    try:
        m.bind_input("x", xs[0].shape)
        m.prepare()
        r = m.clone(ctx2)
        try:
            r.bind_input("x", xs[1].shape)
            r.prepare()
            for mm, cc, x in ((m, ctx, xs[0]), (r, ctx2, xs[1])):
                DeviceTensor(cc, x.shape, np.float32, ptr=mm.input_ptrs["x"], keepalive=mm).upload(x)
            ctx.sync()
            ctx2.sync()
            for _ in range(4):
                m.run(join=False)
                r.run(join=False)
            m.sync()
            r.sync()
            for mm, cc, want, what in ((m, ctx, wants[0], "origin"), (r, ctx2, wants[1], "replica")):
                optr, oshape = mm.output(0)
                bits_equal(DeviceTensor(cc, oshape, np.float32, ptr=optr, keepalive=mm).numpy(), want, what)
        finally:
            r.close()
    finally:
        m.close()
        ctx2.close()
