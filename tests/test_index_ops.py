"""CumSum, GatherElements, Trilu and Tile without a device: the numpy rules (tests/index_rules.py) against the reference's own literals
(tests/golden/index_reference.json); inputs that tell the sequential f32 sum from a chunk-wise one; the Python host operators on a recording context
(launch lists, geometry, every error string, batch coupling, registry); header, ctypes table and Rust bindings; and what `rten_hip_run --parse-only`
prints for, and refuses about, graphs that hold the four nodes."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tests import index_rules as R  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "index_reference.json")))
F, I = np.float32, np.int32
SYMBOLS = ["rten_hip_cumsum_b32", "rten_hip_gather_elements_b32", "rten_hip_trilu_b32", "rten_hip_tile_b32"]
KINDS = ["CumSum", "GatherElements", "Trilu", "Tile"]
# rten_amd/csrc/scan.hip
SCAN_THREADS, SCAN_ROWS, SCAN_CHUNK, SCAN_MAX_BLOCKS = 256, 64, 64, 2048


def _rule_error(f):
    with pytest.raises(R.RuleError) as e:
        f()
    return [e.value.kind, e.value.msg]


# ---------------------------------------------------------------------------------------------- 1. the rules
@pytest.mark.parametrize("case", GOLDEN["cum_sum"], ids=lambda c: c["name"])
def test_cum_sum_rule_matches_reference_literals(case):
    got = R.cum_sum(np.array(case["input"], F).reshape(case["shape"]), case["axis"], case["exclusive"], case["reverse"])
    assert got.dtype == F and got.shape == tuple(case["shape"]) and np.array_equal(got.reshape(-1), np.array(case["expected"], F))


def test_trilu_tile_and_gather_elements_rules_match_reference_literals():
    for case in GOLDEN["trilu"]:
        assert np.array_equal(R.trilu(np.array(case["input"], I), case["k"], case["upper"]), np.array(case["expected"], I)), case["name"]
    for case in GOLDEN["trilu_invalid"]:
        assert _rule_error(lambda: R.trilu(np.array(case["input"], I), case["k"], case["upper"])) == case["error"]
    for case in GOLDEN["tile"]:
        if "input_zeros" in case:
            got = R.tile(np.zeros(case["input_zeros"], I), case["repeats"])
            assert got.shape == tuple(case["expected_zeros"])
        else:
            got = R.tile(np.array(case["input"], I), np.array(case["repeats"], I))
            assert got.dtype == I and np.array_equal(got, np.array(case["expected"], I)) and got.shape == np.array(case["expected"]).shape, case["name"]
    for case in GOLDEN["tile_invalid_repeats"]:
        assert _rule_error(lambda: R.tile(np.array(case["input"], I), case["repeats"])) == case["error"]
    for case in GOLDEN["gather_elements"]:
        got = R.gather_elements(np.array(case["input"], I), np.array(case["indices"], I), case["axis"])
        assert got.dtype == I and np.array_equal(got, np.array(case["expected"], I)), case["name"]
    for case in GOLDEN["gather_elements_invalid_inputs"]:
        assert _rule_error(lambda: R.gather_elements(np.array(case["input"], I), np.array(case["indices"], I), case["axis"])) == case["error"]


def test_cum_sum_rule_edge_values():
    z = R.cum_sum(np.array([-0.0, -0.0, 0.0], F), 0)
    assert not np.signbit(z).any()                                       # +0.0 + -0.0 = +0.0: np.cumsum would keep the -0.0
    assert np.signbit(np.cumsum(np.array([-0.0], F)))[0]
    assert not np.signbit(R.cum_sum(np.array([1.0, -0.0], F), 0, reverse=True)).any()
    assert R.cum_sum(np.array([2 ** 31 - 1, 1, 5], I), 0).tolist() == [2 ** 31 - 1, -2 ** 31, -2 ** 31 + 5]   # int32 wraps
    assert R.cum_sum(np.array([-2 ** 31, -1], I), 0, reverse=True).tolist() == [2 ** 31 - 1, -1]
    x = np.array([[1, np.nan, 2, 3], [1, np.inf, -np.inf, 3], [1, 2, 3, 4]], F)
    y = R.cum_sum(x, 1)
    assert np.isnan(y[0, 1:]).all() and y[0, 0] == 1 and y[1, 1] == np.inf and np.isnan(y[1, 2:]).all() and np.isfinite(y[2]).all()
    y = R.cum_sum(x, 1, reverse=True)                                    # reverse: a NaN reaches what FOLLOWS in walking order, i.e. the lower indices
    assert np.isnan(y[0, :2]).all() and np.isfinite(y[0, 2:]).all()
    y = R.cum_sum(x, 1, exclusive=True)
    assert y[0, 1] == 1 and np.isnan(y[0, 2:]).all()
    assert _rule_error(lambda: R.cum_sum(np.array(1.0, F), 0)) == ["InvalidValue", "Axis is invalid"]   # a rank-0 operand
    assert R.trilu(np.full((2, 2), np.nan, F), 5, True).view(np.uint32).tolist() == [[0, 0], [0, 0]]     # masked NaNs become +0.0
    assert R.gather_elements(np.array([1, 2, 3], I), np.array([3, -4, 2 ** 31 - 1, -2 ** 31], I), 0, clamp=True).tolist() == [3, 1, 3, 1]


def wide_range_lane(n, seed=3):
    """float32 values over six decades: sums in another order round differently."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 10 ** rng.uniform(-3, 3, n)).astype(F)


@pytest.mark.parametrize("n", [2 * SCAN_CHUNK, 2 * SCAN_CHUNK + 1, 5 * SCAN_CHUNK + 7])
def test_inputs_tell_the_sequential_sum_from_a_chunkwise_one(n):
    """The GPU tests use wide_range_lane rows.  A scan that sums within the kernel's chunks and then adds the chunk totals must differ from the rule on them.
    (At SCAN_CHUNK + 1 the later chunk holds ONE element, whose chunk-wise value carry + x is the sequential add itself: no input can differ there, so
    the lengths here are those with several elements in a later chunk.)"""
    x = wide_range_lane(n)
    assert (R.chunked_sum(x, SCAN_CHUNK).view(np.uint32) != R.cum_sum(x, 0).view(np.uint32)).any()
    assert np.array_equal(R.chunked_sum(x[:SCAN_CHUNK + 1], SCAN_CHUNK).view(np.uint32), R.cum_sum(x[:SCAN_CHUNK + 1], 0).view(np.uint32))


# ---------------------------------------------------------------------------------------------- 2. the Python host operators
def _recording():
    from tests.recording_ctx import RecordingCtx

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
        op.run(ctx, inputs)
    assert ctx.calls == []  # refused before anything is launched
    return [e.value.kind, e.value.msg]


def test_python_operators_on_a_recording_context():
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    ctx = _recording()
    t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
    # CumSum: the [outer][axis_len][inner] view of every axis; inner == 1 is the entry point's row form
    x = t(2, 3, 4, 5)
    for axis, view in ((0, (1, 2, 60)), (1, (2, 3, 20)), (-2, (6, 4, 5)), (3, (24, 5, 1)), (-1, (24, 5, 1))):
        for exclusive in (False, True):
            for reverse in (False, True):
                del ctx.calls[:]
                y = ops.CumSum(exclusive, reverse).run(ctx, [x, np.array(axis, I)])[0]
                (name, args), = ctx.calls
                assert y.shape == x.shape and y.dtype == F and name == "rten_hip_cumsum_b32"
                assert list(args[:6]) == [0, int(exclusive), int(reverse), *view] and [a.value for a in args[6:]] == [x.ptr, y.ptr]
    del ctx.calls[:]
    xi = t(7, 9, dtype=I)
    y = ops.CumSum().run(ctx, [xi, np.array([1], np.int64)])[0]  # one element of any rank, as the reference's require_as::<i32>
    assert y.dtype == I and list(ctx.calls[0][1][:6]) == [1, 0, 0, 7, 9, 1]
    del ctx.calls[:]
    assert ops.CumSum().run(ctx, [t(3, 0, 5), np.array(1, I)])[0].shape == (3, 0, 5) and ctx.calls == []  # an empty tensor launches nothing
    assert ops.CumSum().exclusive is False and ops.CumSum().reverse is False and ops.CumSum().max_inputs() == 2
    assert ops.CumSum().batch_coupled((4, 5), 0) and ops.CumSum().batch_coupled((4, 5), -2) and not ops.CumSum().batch_coupled((4, 5), 1)

    # GatherElements: the output has the indices' shape and the data's dtype; the axis is resolved on the host
    for dtype in (F, I):
        x, ids = t(4, 5, 6, dtype=dtype), t(3, 5, 2, dtype=I)
        for axis, ax in ((1, 1), (-2, 1)):
            del ctx.calls[:]
            y = ops.GatherElements(axis).run(ctx, [x, ids])[0]
            (name, args), = ctx.calls
            assert y.shape == (3, 5, 2) and y.dtype == dtype and name == "rten_hip_gather_elements_b32"
            assert args[0] == 3 and tuple(args[1]) == (4, 5, 6) and tuple(args[2]) == (3, 5, 2) and args[3] == ax
            assert isinstance(args[1], C.Array) and args[1]._type_ is C.c_int64 and [a.value for a in args[4:]] == [x.ptr, ids.ptr, y.ptr]
    del ctx.calls[:]
    assert ops.GatherElements(0).run(ctx, [t(3), t(0, dtype=I)])[0].shape == (0,) and ctx.calls == []
    y = ops.GatherElements(0).run(ctx, [t(3), np.array([-3, 2, 0], I)])[0]  # host-side indices in range: uploaded, then one launch
    assert y.shape == (3,) and [c[0] for c in ctx.calls][-1] == "rten_hip_gather_elements_b32"
    assert ops.GatherElements().axis == 0 and ops.GatherElements().max_inputs() == 2
    assert ops.GatherElements(0).batch_coupled((4, 5)) and ops.GatherElements(-2).batch_coupled((4, 5)) and not ops.GatherElements(1).batch_coupled((4, 5))

    # Trilu: [batch][rows][cols]; k optional
    for upper in (True, False):
        for k_in, k in ((None, 0), (np.array(-3, I), -3), (np.array([7], np.int64), 7)):
            del ctx.calls[:]
            x = t(2, 3, 5, 7, dtype=I)
            y = ops.Trilu(upper).run(ctx, [x] if k_in is None else [x, k_in])[0]
            (name, args), = ctx.calls
            assert y.shape == x.shape and y.dtype == I and name == "rten_hip_trilu_b32"
            assert list(args[:5]) == [int(upper), k, 6, 5, 7] and [a.value for a in args[5:]] == [x.ptr, y.ptr]
    del ctx.calls[:]
    assert ops.Trilu().run(ctx, [t(5, 7)])[0].shape == (5, 7) and list(ctx.calls[0][1][:5]) == [1, 0, 1, 5, 7]
    del ctx.calls[:]
    assert ops.Trilu().run(ctx, [t(2, 0, 7)])[0].shape == (2, 0, 7) and ctx.calls == []
    assert ops.Trilu().upper is True and ops.Trilu().max_inputs() == 2
    assert ops.Trilu().batch_coupled((5, 7)) and not ops.Trilu().batch_coupled((2, 5, 7))

    # Tile
    del ctx.calls[:]
    x = t(2, 3, 4)
    y = ops.Tile().run(ctx, [x, np.array([1, 3, 2], np.int64)])[0]
    (name, args), = ctx.calls
    assert y.shape == (2, 9, 8) and name == "rten_hip_tile_b32" and args[0] == 3 and tuple(args[1]) == (2, 3, 4) and tuple(args[2]) == (1, 3, 2)
    assert args[1]._type_ is C.c_int64 and args[2]._type_ is C.c_int64 and [a.value for a in args[3:]] == [x.ptr, y.ptr]
    del ctx.calls[:]
    assert ops.Tile().run(ctx, [t(3, 4, 5), np.array([4, 0, 1], I)])[0].shape == (12, 0, 5) and ctx.calls == []  # a zero repeat: an empty output, no launch
    y = ops.Tile().run(ctx, [t(dtype=I), np.zeros(0, I)])[0]  # a scalar with no repeats: one element
    assert y.shape == () and len(ctx.calls) == 1 and ctx.calls[0][1][0] == 0
    assert ops.Tile().max_inputs() == 2
    assert ops.Tile.batch_coupled([2, 1]) and not ops.Tile.batch_coupled([1, 3]) and not ops.Tile.batch_coupled([])

    reg = ops.OpRegistry.with_all_ops()
    for kind in KINDS:
        assert reg.get(kind) is getattr(ops, kind)


def test_python_operator_errors():
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    ctx = _recording()
    t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
    axis = np.array(0, I)
    assert _refusal(ops.CumSum(), [t(), axis]) == ["InvalidValue", "Axis is invalid"]  # a rank-0 operand: the reference's axis error
    assert _refusal(ops.CumSum(), [t(2, 3), np.array(2, I)]) == ["InvalidValue", "Axis is invalid"]
    assert _refusal(ops.CumSum(), [t(2, 3), np.array(-3, I)]) == ["InvalidValue", "Axis is invalid"]
    assert _refusal(ops.CumSum(), [t(2, 3)])[0] == "MissingInputs"
    assert _refusal(ops.CumSum(), [t(2, 3), np.array([0, 1], I)]) == ["InputCastFailed", "expected tensor with 0 dims"]
    assert _refusal(ops.CumSum(), [t(2, 3), np.array(0.0, F)]) == ["InputCastFailed", "expected int32 tensor"]
    assert _refusal(ops.CumSum(), [t(2, 3, dtype=np.uint8), axis])[0] == "UnsupportedType"

    for case in GOLDEN["gather_elements_invalid_inputs"]:
        x, ids = np.array(case["input"], I), np.array(case["indices"], I)
        assert _refusal(ops.GatherElements(case["axis"]), [t(*x.shape, dtype=I), ids]) == case["error"], case["name"]  # host-valued indices: the reference's message
    assert _refusal(ops.GatherElements(0), [t(3), np.array([-4], I)]) == ["InvalidValue", "Entry in `indices` is out of range"]
    assert _refusal(ops.GatherElements(0), [t(0), t(2, dtype=I)]) == ["InvalidValue", "Entry in `indices` is out of range"]  # an empty axis: nothing to clamp to
    assert _refusal(ops.GatherElements(0), [t(3), t(3)]) == ["InputCastFailed", "expected int32 tensor"]
    assert _refusal(ops.GatherElements(0), [t(3, dtype=np.uint8), t(3, dtype=I)])[0] == "UnsupportedType"
    assert _refusal(ops.GatherElements(0), [t(1, 1, 1, 1, 1, 1, 2), t(1, 1, 1, 1, 1, 1, 2, dtype=I)])[0] == "UnsupportedValue"
    assert _refusal(ops.GatherElements(0), [t(3)])[0] == "MissingInputs"

    for case in GOLDEN["trilu_invalid"]:
        assert _refusal(ops.Trilu(case["upper"]), [t(len(case["input"]), dtype=I)]) == case["error"]
    assert _refusal(ops.Trilu(), [t()]) == ["InvalidValue", "Input must have >= 2 dims"]
    assert _refusal(ops.Trilu(), [t(2, 2), np.array([1, 2], I)]) == ["InputCastFailed", "expected tensor with 0 dims"]
    assert _refusal(ops.Trilu(), [t(2, 2, dtype=np.int8)])[0] == "UnsupportedType"
    assert _refusal(ops.Trilu(), [])[0] == "MissingInputs"

    for case in GOLDEN["tile_invalid_repeats"]:
        assert _refusal(ops.Tile(), [t(len(case["input"]), dtype=I), np.array(case["repeats"], I)]) == case["error"]
    assert _refusal(ops.Tile(), [t(2, 2), np.array([[1, 1]], I)]) == ["InputCastFailed", "expected tensor with 1 dims"]
    assert _refusal(ops.Tile(), [t(2, 2), np.array([1.0, 1.0], F)]) == ["InputCastFailed", "expected int32 tensor"]
    assert _refusal(ops.Tile(), [t(2, 2)])[0] == "MissingInputs"
    assert _refusal(ops.Tile(), [t(1, 1, 1, 1, 1, 1, 2), np.ones(7, I)])[0] == "UnsupportedValue"


# ---------------------------------------------------------------------------------------------- 3. header, ctypes, bindings
def test_header_ctypes_and_bindings_carry_the_symbols():
    from rten_amd import lib as L
    header = open(os.path.join(ROOT, "include", "rten_hip.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "rten-hip-sys", "src", "lib.rs")).read()
    assert "#define RTEN_HIP_ABI_VERSION 8\n" in header  # additive: the version stays
    for sym in SYMBOLS:
        assert re.search(r"int32_t " + sym + r"\(rten_hip_ctx \*ctx", header), sym
        assert sym in L.PROTOTYPES and L.PROTOTYPES[sym][0] is C.c_int32, sym
        assert f"pub fn {sym}(ctx: *mut rten_hip_ctx" in bindings, sym
    assert len(L.PROTOTYPES["rten_hip_cumsum_b32"][1]) == 9 and len(L.PROTOTYPES["rten_hip_gather_elements_b32"][1]) == 8
    assert len(L.PROTOTYPES["rten_hip_trilu_b32"][1]) == 8 and len(L.PROTOTYPES["rten_hip_tile_b32"][1]) == 6
    assert "k: i64" in bindings[bindings.index("pub fn rten_hip_trilu_b32"):].split("\n")[0]
    ops_header = open(os.path.join(ROOT, "include", "rten_hip_ops.hpp")).read()
    for kind in KINDS:
        assert f'r.register_op<{kind}>("{kind}");' in ops_header, kind
    kernels = open(os.path.join(ROOT, "rten_amd", "csrc", "scan.hip")).read()  # the geometry the GPU tests mirror
    for name, v in (("SCAN_THREADS", SCAN_THREADS), ("SCAN_ROWS", SCAN_ROWS), ("SCAN_CHUNK", SCAN_CHUNK), ("SCAN_MAX_BLOCKS", SCAN_MAX_BLOCKS)):
        assert re.search(r"constexpr (int|int64_t) " + name + r" = " + str(v) + r";", kernels), name
    assert "asm" not in kernels


# ---------------------------------------------------------------------------------------------- 4. the loader's checks, through the CLI
def _parse_only(tmp_path, name, data):
    from tests.test_graph_executor import run_cli
    p = tmp_path / name
    p.write_bytes(data)
    return run_cli("--parse-only", str(p))


def _index_lines(out):
    return [ln.strip() for ln in out.stdout.splitlines() if ln.strip().startswith("index step")]


@pytest.mark.parametrize("dynamic", [False, True])
def test_cli_parses_the_exported_graphs(tmp_path, dynamic):
    """Fails on a tree without the four operators: its --parse-only prints no `index step` line (and its loader refuses the graphs at the CumSum node:
    "operator CumSum is not available on the HIP backend")."""
    import torch_export as te
    out = _parse_only(tmp_path, "roberta.onnx", te.roberta_onnx(dynamic=dynamic))
    assert out.returncode == 0, out.stderr
    lines = _index_lines(out)
    assert "producer pytorch" in out.stdout and "CumSum x1" in out.stdout and "GatherElements x1" in out.stdout, out.stdout
    assert len(lines) == 2 and re.fullmatch(r'index step CumSum "[^"]+": exclusive 0, reverse 0, axis from input 1 \(a host value at run time\)', lines[0]), lines
    assert re.fullmatch(r'index step GatherElements "[^"]+": axis 1', lines[1]), lines
    out = _parse_only(tmp_path, "decoder.onnx", te.causal_decoder_onnx(dynamic=dynamic))
    assert out.returncode == 0, out.stderr
    lines = _index_lines(out)
    for kind in KINDS:
        assert f"{kind} x1" in out.stdout, out.stdout
    assert [ln.split()[2] for ln in lines] == ["CumSum", "Trilu", "GatherElements", "Tile"], lines
    assert re.fullmatch(r'index step Trilu "[^"]+": upper, k from input 1 \(a host value at run time\)', lines[1]), lines
    assert re.fullmatch(r'index step Tile "[^"]+": repeats from input 1 \(a host value at run time\)', lines[3]), lines


def test_cli_parses_the_writer_graph_with_every_attribute(tmp_path):
    from rten_amd import onnx_writer as ow
    out = _parse_only(tmp_path, "index.onnx", ow.index_ops_graph())
    assert out.returncode == 0, out.stderr
    assert _index_lines(out) == ['index step CumSum "cum_excl_rev": exclusive 1, reverse 1, axis from input 1 (a host value at run time)',
                                 'index step CumSum "cum_mid_rev": exclusive 0, reverse 1, axis from input 1 (a host value at run time)',
                                 'index step CumSum "cum_int_excl": exclusive 1, reverse 0, axis from input 1 (a host value at run time)',
                                 'index step CumSum "cum_rows": exclusive 0, reverse 0, axis from input 1 (a host value at run time)',
                                 'index step GatherElements "gather_mid": axis 1', 'index step GatherElements "gather_last": axis -1',
                                 'index step Trilu "tril_km1": lower, k from input 1 (a host value at run time)',
                                 'index step Trilu "triu_k1": upper, k from input 1 (a host value at run time)',
                                 'index step Tile "tiled": repeats from input 1 (a host value at run time)']
    x = [ow.value_info("x", ow.FLOAT, [2, 3, 3])]
    out = _parse_only(tmp_path, "default_k.onnx", ow.model([ow.node("Trilu", ["x"], ["y"], name="mask")], x, [ow.value_info("y", ow.FLOAT, [2, 3, 3])], [], opset=14))
    assert out.returncode == 0 and _index_lines(out) == ['index step Trilu "mask": upper, k 0'], out.stdout + out.stderr  # upper defaults to 1, k to 0
    out = _parse_only(tmp_path, "default_axis.onnx", ow.model([ow.node("GatherElements", ["x", "x"], ["y"], name="pick")], x, [ow.value_info("y", ow.FLOAT, [2, 3, 3])], []))
    assert out.returncode == 0 and _index_lines(out) == ['index step GatherElements "pick": axis 0'], out.stdout + out.stderr


@pytest.mark.parametrize("bad,words", [("cumsum_no_axis", ("CumSum cum_rows", "the axis input is missing")),
                                       ("cumsum_axis_input", ("CumSum cum_rows", "axis must be a constant or computable from the input shapes", '"axis_in"')),
                                       ("trilu_k_input", ("Trilu triu_k1", "k must be a constant or computable from the input shapes", '"k_in"')),
                                       ("tile_repeats_input", ("Tile tiled", "repeats must be a constant or computable from the input shapes", '"repeats_in"')),
                                       ("trilu_extra_input", ("Trilu triu_k1", "takes at most 2 inputs (it has 3)")),
                                       ("tile_extra_input", ("Tile tiled", "takes at most 2 inputs (it has 3)"))])
def test_cli_refuses_by_node_name(tmp_path, bad, words):
    from rten_amd import onnx_writer as ow
    out = _parse_only(tmp_path, "bad.onnx", ow.index_ops_graph(bad=bad))
    assert out.returncode == 1 and all(w in out.stderr for w in words), out.stdout + out.stderr
