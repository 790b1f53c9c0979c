"""DFT and STFT without a GPU: the rules file (tests/fft_rules.py) against every literal of the reference's test_stft / test_dft
(tests/golden/fft_reference.json, within 1e-4), the host-only pass planner rten_hip_fft_plan, both registries, the Python operators on a recording context
(shapes, default n_fft, the arguments of the launch, every error string of the golden file, refused before anything is launched), the header's additions with
the ABI version unchanged, and the builder graphs through the loader's --parse-only checks."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import fft_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "fft_reference.json")))
GPU_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 12, 15, 16, 25, 30, 31, 37, 49, 64, 97, 100, 128, 400, 512, 1000, 1024, 4096, 8192]


def _dft_case_arrays(case):
    x = np.asarray(case["input"], F).reshape(case.get("input_shape", np.asarray(case["input"]).shape))
    want = None
    if "expected" in case:
        want = np.asarray(case["expected"], np.float64).reshape(case.get("expected_shape", np.asarray(case["expected"]).shape))
    return x, want


# ---------------------------------------------------------------------------------------------- 1. the rules against the reference's literals
@pytest.mark.parametrize("case", GOLDEN["dft"], ids=lambda c: c["name"])
def test_dft_rule_reproduces_the_reference_literals(case):
    x, want = _dft_case_arrays(case)
    args = (case["dft_length"], case["axis"], case["inverse"], case["onesided"])
    if "error" in case:
        assert ["InvalidValue", R.dft_error(x.shape, *args)] == case["error"]
        with pytest.raises(ValueError):
            R.dft(x, *args)
        return
    got = R.dft(x, *args)
    assert got.shape == want.shape and got.dtype == np.float64 and np.abs(got - want).max() <= GOLDEN["tolerance"]


@pytest.mark.parametrize("case", GOLDEN["stft"], ids=lambda c: c["name"])
def test_stft_rule_reproduces_the_reference_literals(case):
    signal = np.asarray(case["signal"], F)
    window = None if case["window"] is None else np.asarray(case["window"], F)
    if "error" in case:
        err = R.stft_error(signal.shape, case["frame_step"], None if window is None else len(window), case["frame_length"], case["onesided"])
        assert ["InvalidValue", err] == case["error"]
        return
    got = R.stft(signal, case["frame_step"], window, case["frame_length"], case["onesided"])
    want = np.asarray(case["expected"], np.float64)
    assert got.shape == want.shape and np.abs(got - want).max() <= GOLDEN["tolerance"]


def test_rules_follow_the_loader_and_storer_rules():
    rng = np.random.default_rng(3)
    # IRFFT: the conjugate half is rebuilt from bins 1 .. conj_end - 1; for even N the Nyquist bin is left as given, imaginary part included
    half = rng.standard_normal((2, 5, 2)).astype(F)
    full = np.zeros((2, 8), np.complex128)
    z = half[..., 0].astype(np.float64) + 1j * half[..., 1]
    full[:, :5] = z
    for k in (1, 2, 3):
        full[:, 8 - k] = np.conj(z[:, k])
    want = (np.fft.ifft(full, axis=-1) * 8 * float(F(1) / F(8))).real
    assert np.allclose(R.dft(half, None, -2, True, True)[..., 0], want, rtol=0, atol=1e-15)
    # odd N: conj_end = n_in, so the last given bin is mirrored too; bins at k >= n_in are zero
    odd = R.dft(half[:, :3], 7, -2, True, True)
    full = np.zeros((2, 7), np.complex128)
    full[:, :3] = z[:, :3]
    full[:, 6], full[:, 5] = np.conj(z[:, 1]), np.conj(z[:, 2])
    assert np.allclose(odd[..., 0], (np.fft.ifft(full, axis=-1) * 7 * float(F(1) / F(7))).real, rtol=0, atol=1e-15)
    # the default length of IRFFT saturates at 0; a one-sided forward transform of nothing is one zero bin
    assert R.dft(np.zeros((2, 1, 2), F), None, -2, True, True).shape == (2, 0, 1)
    assert R.dft(np.zeros((2, 0, 1), F), None, -2, False, True).shape == (2, 1, 2)
    # STFT forms window * signal in float32 before widening
    s, w = rng.standard_normal((1, 9)).astype(F), rng.standard_normal(4).astype(F)
    got = R.stft(s, 5, w, None, False)
    assert got.shape == (1, 2, 4, 2)
    assert np.array_equal(got[0, 1, :, 0] + 1j * got[0, 1, :, 1], np.fft.fft((w * s[0, 5:9]).astype(np.float64)))
    # an all-zero lane must be exactly zero: the ratio is inf otherwise, whatever the bound
    want = np.zeros((2, 4, 2))
    want[1] = 1.0
    got = want.astype(F)
    got[0, 2, 1] = 1e-30
    r = R.lane_ratios(got, want, 4)
    assert np.isinf(r[0]) and r[1] == 0.0


# ---------------------------------------------------------------------------------------------- 2. the pass planner
def test_plan_factors_every_length_in_the_stated_order():
    from rten_amd import lib as L
    assert L.FFT_MAX == 8192 and L.FFT_GENERIC_RADIX_MAX == 31
    small_primes = [p for p in range(2, 32) if all(p % q for q in range(2, p))]
    for n in sorted(set(GPU_LENGTHS + list(range(1, 130)) + [961, 2187, 3125, 7 * 11 * 13, 8190])):
        plan = L.fft_plan(n)
        assert int(np.prod(plan, dtype=np.int64)) == n, (n, plan)
        if len(plan) == 1 and plan[0] > 31:
            assert max(p for p in range(2, n + 1) if n % p == 0 and all(p % q for q in range(2, int(p ** 0.5) + 1))) > 31, n  # a prime factor above 31: one direct pass
            continue
        assert all(r == 4 or r in small_primes for r in plan), (n, plan)
        assert plan.count(2) <= 1 and (2 not in plan or 4 not in plan or plan.index(2) > max(i for i, r in enumerate(plan) if r == 4)), (n, plan)  # 4s before the 2
        rest = [r for r in plan if r not in (4, 2)]
        assert rest == sorted(rest), (n, plan)  # then 3s, 5s, then the generic primes
    assert L.fft_plan(1) == [] and L.fft_plan(8) == [4, 2] and L.fft_plan(400) == [4, 4, 5, 5] and L.fft_plan(49) == [7, 7] and L.fft_plan(31) == [31]
    for n in (37, 97, 8191, 2 * 37, 4 * 41):
        assert L.fft_plan(n) == [n], n  # a single direct pass of radix n
    with pytest.raises(ValueError, match="above the limit of 8192"):
        L.fft_plan(8193)
    with pytest.raises(ValueError):
        L.fft_plan(0)
    buf = (C.c_int32 * 16)()
    so = L.load()
    assert so.rten_hip_fft_plan(8193, buf, 16) == -L.ERR_UNSUPPORTED and so.rten_hip_fft_plan(400, buf, 3) == -L.ERR_INVALID_VALUE and so.rten_hip_fft_plan(400, None, 16) == -L.ERR_INVALID_VALUE
    assert R.bound_constant(400) == 2 + 14 + 14 + 16 + 16 and R.bound_constant(1) == 2 and R.bound_constant(37) == 2 + 80


# ---------------------------------------------------------------------------------------------- 3. registries, header, ctypes, bindings
def test_both_registries_header_ctypes_and_bindings_carry_the_operators():
    from rten_amd import lib as L
    from rten_amd import ops
    types = ops.OpRegistry.with_all_ops().op_types()
    assert "DFT" in types and "STFT" in types and ops.DFT().max_inputs() == 3 and ops.STFT().max_inputs() == 4
    assert ops.STFT().onesided and not ops.DFT().inverse and not ops.DFT().onesided
    ops_header = open(os.path.join(ROOT, "include", "rten_hip_ops.hpp")).read()
    assert 'r.register_op<DFT>("DFT");' in ops_header and 'r.register_op<STFT>("STFT");' in ops_header
    header = open(os.path.join(ROOT, "include", "rten_hip.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "rten-hip-sys", "src", "lib.rs")).read()
    assert "#define RTEN_HIP_ABI_VERSION 8\n" in header  # additive: the version stays
    assert "#define RTEN_HIP_FFT_MAX 8192\n" in header and "#define RTEN_HIP_FFT_GENERIC_RADIX_MAX 31\n" in header
    for sym, nargs in (("rten_hip_dft_f32", 9), ("rten_hip_stft_f32", 10), ("rten_hip_fft_plan", 3)):
        assert re.search(r"int32_t " + sym + r"\(", header), sym
        assert sym in L.PROTOTYPES and L.PROTOTYPES[sym][0] is C.c_int32 and len(L.PROTOTYPES[sym][1]) == nargs, sym
        assert f"pub fn {sym}(" in bindings, sym
        assert hasattr(L.load(), sym)
    line = bindings[bindings.index("pub fn rten_hip_stft_f32("):].split("\n")[0]
    assert "frame_step: i64" in line and "window_or_null: *const f32" in line and "signal: *const f32" in line, line
    comment = header[header.index("/* DFT and STFT"):header.index("int32_t rten_hip_dft_f32")]
    for case in GOLDEN["dft"] + GOLDEN["stft"]:
        if "error" in case and case["error"][1] not in ("dft_length must be >= 1", "Either frame_length or window must be set", "window length must equal frame_length"):
            assert case["error"][1] in comment, case["error"][1]  # (those three are the host operators' alone: the entry points take n_fft)


# ---------------------------------------------------------------------------------------------- 4. the Python operators
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


def _refusal(op, inputs):
    from rten_amd import ops
    ctx = _recording()
    with pytest.raises(ops.OpError) as e:
        op.run(ctx, inputs(ctx))
    assert ctx.calls == []  # refused before anything is launched
    return [e.value.kind, e.value.msg]


def _val(a):
    return a.value if hasattr(a, "value") else a


def test_python_dft_shapes_default_lengths_and_launch_arguments():
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    ctx = _recording()
    t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
    i64 = lambda v: np.array(v, np.int64)
    for shape, inputs, flags, out, launch in (
            ((3, 12, 2), [], (0, 0), (3, 12, 2), [3, 12, 12, 2, 0, 0]),
            ((3, 12, 1), [], (0, 1), (3, 7, 2), [3, 12, 12, 1, 0, 1]),
            ((3, 7, 2), [], (1, 1), (3, 12, 1), [3, 7, 12, 2, 1, 1]),       # IRFFT: 2 * (7 - 1)
            ((3, 1, 2), [i64(5)], (1, 1), (3, 5, 1), [3, 1, 5, 2, 1, 1]),
            ((3, 12, 2), [i64([20])], (1, 0), (3, 20, 2), [3, 12, 20, 2, 1, 0]),
            ((3, 12, 1), [i64(5), i64(-2)], (0, 1), (3, 3, 2), [3, 12, 5, 1, 0, 1]),
            ((2, 3, 12, 1), [None, i64(2)], (0, 0), (2, 3, 12, 2), [6, 12, 12, 1, 0, 0])):
        del ctx.calls[:]
        y = ops.DFT(*flags).run(ctx, [t(*shape)] + inputs)[0]
        (name, args), = ctx.calls
        assert name == "rten_hip_dft_f32" and y.shape == out and [_val(a) for a in args[:6]] == launch, (shape, flags)
    # another axis: transpose, transform, transpose back; the output takes the input's axis order
    del ctx.calls[:]
    y = ops.DFT(False, True).run(ctx, [t(1, 4, 2, 1), None, i64(1)])[0]
    assert y.shape == (1, 3, 2, 2) and [c[0] for c in ctx.calls] == ["rten_hip_transpose_b32", "rten_hip_dft_f32", "rten_hip_transpose_b32"]
    assert [_val(a) for a in ctx.calls[1][1][:6]] == [2, 4, 4, 1, 0, 1]
    del ctx.calls[:]
    y = ops.DFT().run(ctx, [t(6, 3, 5, 2), i64(9), i64(-4)])[0]
    assert y.shape == (9, 3, 5, 2) and [_val(a) for a in ctx.calls[1][1][:6]] == [15, 6, 9, 2, 0, 0]
    assert ops.DFT().batch_coupled((6, 3, 5, 2), -4) and ops.DFT().batch_coupled((6, 2), 0) and not ops.DFT().batch_coupled((6, 3, 2))
    # IRFFT of an empty spectrum: the default length saturates at 0, nothing is launched; a one-sided transform of nothing is one bin, zero-filled by the entry point
    del ctx.calls[:]
    assert ops.DFT(True, True).run(ctx, [t(3, 0, 2)])[0].shape == (3, 0, 1) and ctx.calls == []
    assert ops.DFT(False, True).run(ctx, [t(3, 0, 1)])[0].shape == (3, 1, 2) and [_val(a) for a in ctx.calls[0][1][:3]] == [3, 0, 0]


def test_python_stft_shapes_and_launch_arguments():
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    ctx = _recording()
    t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
    i64 = lambda v: np.array(v, np.int64)
    for signal, inputs, onesided, out, launch in (
            ((2, 100), [i64(10), t(16)], True, (2, 9, 9, 2), [2, 100, 1, 10, 16, 1]),
            ((2, 100, 1), [i64([10]), None, i64(16)], True, (2, 9, 9, 2), [2, 100, 1, 10, 16, 1]),
            ((2, 100, 2), [i64(7), t(16), i64(16)], False, (2, 13, 16, 2), [2, 100, 2, 7, 16, 0]),
            ((2, 100), [i64(200), t(100)], False, (2, 1, 100, 2), [2, 100, 1, 200, 100, 0]),
            ((2, 100), [i64(1), None, i64(1)], True, (2, 100, 1, 2), [2, 100, 1, 1, 1, 1])):
        del ctx.calls[:]
        y = ops.STFT(onesided).run(ctx, [t(*signal)] + inputs)[0]
        (name, args), = ctx.calls
        assert name == "rten_hip_stft_f32" and y.shape == out and [_val(a) for a in args[:6]] == launch, (signal, onesided)
        assert (args[6] is None) == (len(inputs) < 2 or inputs[1] is None)
    del ctx.calls[:]
    assert ops.STFT().run(ctx, [t(0, 100), i64(10), t(16)])[0].shape == (0, 9, 9, 2) and ctx.calls == []


def test_python_operators_refuse_with_the_reference_s_strings():
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    i64 = lambda v: np.array(v, np.int64)
    for case in GOLDEN["dft"]:
        if "error" not in case:
            continue
        x, _ = _dft_case_arrays(case)
        extra = [None if case["dft_length"] is None else i64(case["dft_length"]), i64(case["axis"])]
        assert _refusal(ops.DFT(case["inverse"], case["onesided"]), lambda c: [DeviceTensor(c, x.shape, F)] + extra) == case["error"], case["name"]
    for case in GOLDEN["stft"]:
        if "error" not in case:
            continue
        shape = np.asarray(case["signal"]).shape
        inputs = lambda c: [DeviceTensor(c, shape, F), i64(case["frame_step"]), None if case["window"] is None else DeviceTensor(c, (len(case["window"]),), F),
                            None if case["frame_length"] is None else i64(case["frame_length"])]
        assert _refusal(ops.STFT(case["onesided"]), inputs) == case["error"], case["name"]
    for case in GOLDEN["messages_without_a_literal_case"]:
        if case["op"] == "DFT":
            got = _refusal(ops.DFT(), lambda c: [DeviceTensor(c, case["input_shape"], F), None, i64(case.get("axis", -2))])
        else:
            got = _refusal(ops.STFT(case.get("onesided", True)), lambda c: [DeviceTensor(c, case["input_shape"], F), i64(case["frame_step"]), None, i64(case["frame_length"])])
        assert got == case["error"], case["name"]
    ok = lambda c: [DeviceTensor(c, (2, 8, 1), F)]
    assert _refusal(ops.DFT(), lambda c: []) == ["MissingInputs", ""]
    assert _refusal(ops.DFT(), lambda c: [DeviceTensor(c, (2, 8, 1), I)]) == ["InputCastFailed", "expected float32 tensor"]
    assert _refusal(ops.DFT(), lambda c: ok(c) + [i64([4, 4])]) == ["InputCastFailed", "expected tensor with 0 dims"]
    assert _refusal(ops.DFT(), lambda c: ok(c) + [np.array(4.0, F)]) == ["InputCastFailed", "expected int32 tensor"]
    assert _refusal(ops.DFT(), lambda c: ok(c) + [None, i64(3)]) == ["InvalidValue", "Axis is invalid"]
    assert _refusal(ops.DFT(), lambda c: ok(c) + [i64(8193)]) == ["UnsupportedValue", "DFT transform of length 8193 exceeds the limit of 8192 points (RTEN_HIP_FFT_MAX)"]
    assert _refusal(ops.STFT(), lambda c: [DeviceTensor(c, (1, 9000), F), i64(1), None, i64(8193)]) == \
        ["UnsupportedValue", "STFT frame of length 8193 exceeds the limit of 8192 points (RTEN_HIP_FFT_MAX)"]
    assert _refusal(ops.STFT(), lambda c: [DeviceTensor(c, (1, 8), F)]) == ["MissingInputs", ""]
    assert _refusal(ops.STFT(), lambda c: [DeviceTensor(c, (1, 8), F), i64(2), DeviceTensor(c, (9,), F)]) == ["InvalidValue", "frame_length must be in range [1, signal_length]"]
    for op, inputs, what in ((ops.DFT(), lambda c: ok(c) + [DeviceTensor(c, (1,), I)], "dft_length"), (ops.DFT(), lambda c: ok(c) + [None, DeviceTensor(c, (), I)], "axis"),
                             (ops.STFT(), lambda c: ok(c) + [DeviceTensor(c, (), I), None, i64(4)], "frame_step"),
                             (ops.STFT(), lambda c: ok(c) + [i64(2), None, DeviceTensor(c, (1,), I)], "frame_length")):
        kind, msg = _refusal(op, inputs)
        assert kind == "UnsupportedValue" and what in msg and "device data" in msg, msg


# ---------------------------------------------------------------------------------------------- 5. the builder graphs, through the loader's checks
def _parse_only(tmp_path, name, data):
    from tests.test_graph_executor import run_cli
    p = tmp_path / name
    p.write_bytes(data)
    return run_cli("--parse-only", str(p))


def _fft_lines(out):
    return [ln.strip() for ln in out.stdout.splitlines() if ln.strip().startswith("fft step")]


def test_builder_graphs_parse_and_print_their_step_lines(tmp_path):
    """Fails on a tree without the operators: its --parse-only prints no `fft step` line (and its loader refuses the graphs: "operator STFT is not available on
    the HIP backend (no CPU fallback)")."""
    from rten_amd import onnx_writer as ow
    out = _parse_only(tmp_path, "log_mel.onnx", ow.log_mel_graph(expose_stft=True)[0])
    assert out.returncode == 0 and "STFT x1" in out.stdout, out.stdout + out.stderr
    assert _fft_lines(out) == ['fft step "stft": STFT onesided 1, window from input 2, frame_length the window\'s length'], out.stdout
    out = _parse_only(tmp_path, "dft17.onnx", ow.dft_graph(opset=17)[0])
    assert out.returncode == 0 and _fft_lines(out) == ['fft step "forward": DFT inverse 0, onesided 0, axis 1', 'fft step "inverse": DFT inverse 1, onesided 0, axis 1'], out.stdout
    out = _parse_only(tmp_path, "dft20.onnx", ow.dft_graph(opset=20, dft_length=16)[0])
    assert out.returncode == 0 and _fft_lines(out) == ['fft step "forward": DFT inverse 0, onesided 0, axis from input 2',
                                                       'fft step "inverse": DFT inverse 1, onesided 0, axis from input 2'], out.stdout


def test_loader_refuses_by_node_name_under_parse_only(tmp_path):
    from rten_amd import onnx_writer as ow
    FLOAT, INT64 = ow.FLOAT, ow.INT64
    x = [ow.value_info("x", FLOAT, ["batch", 64])]
    y = [ow.value_info("y", FLOAT, ["batch", "frames", 9, 2])]
    hop = ow.tensor("hop", np.asarray(4, np.int64))
    for nodes, ins, inits, words in (
            ([ow.node("STFT", ["x", "hop"], ["y"], name="front/stft")], x, [hop], ("STFT front/stft", "Either frame_length or window must be set")),
            ([ow.node("STFT", ["x", "step", "", "hop"], ["y"], name="front/stft")], x + [ow.value_info("step", INT64, [])], [hop],
             ("STFT front/stft", "frame_step must be a constant or computable from the input shapes", '"step"')),
            ([ow.node("STFT", ["x", "hop", "", "hop", "hop"], ["y"], name="front/stft")], x, [hop], ("STFT front/stft", "takes at most 4 inputs (it has 5)")),
            ([ow.node("DFT", ["x3", "n"], ["y"], name="spec/dft")], [ow.value_info("x3", FLOAT, ["batch", 8, 1]), ow.value_info("n", INT64, [])], [],
             ("DFT spec/dft", "dft_length must be a constant or computable from the input shapes", '"n"')),
            ([ow.node("DFT", ["x3", "", "hop", "hop"], ["y"], name="spec/dft")], [ow.value_info("x3", FLOAT, ["batch", 8, 1])], [hop], ("DFT spec/dft", "takes at most 3 inputs (it has 4)"))):
        out = _parse_only(tmp_path, "bad.onnx", ow.model(nodes, ins, y, inits, opset=20))
        assert out.returncode != 0, out.stdout
        for w in words:
            assert w in out.stderr + out.stdout, (w, out.stderr[-800:])


def test_exported_log_mel_module_is_the_graph_the_issue_names(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export
    data, w = torch_export.log_mel_onnx(n_mels=20)
    out = _parse_only(tmp_path, "torch_log_mel.onnx", data)
    assert out.returncode == 0, out.stdout + out.stderr
    for op in ("Shape", "Gather", "Unsqueeze", "Concat", "Reshape", "Pad", "STFT x1", "Transpose", "Pow", "Add", "MatMul", "Clip", "Log", "Div", "ReduceMax", "Sub", "Max"):
        assert op in out.stdout, op
    (line,) = _fft_lines(out)
    assert "STFT onesided 1, window from input 2, frame_length from input 3" in line
    assert w["window"].shape == (400,) and w["mel"].shape == (201, 20)
