"""GridSample and DepthToSpace without a device: the numpy rules (tests/sample_rules.py) against the reference's own literals
(tests/golden/sample_reference.json), torch and the ONNX specification; the Python host operators on a recording context (arguments, the single
transpose launch, errors, registry); and what `rten_hip_run --parse-only` prints for, and refuses about, graphs that hold the two nodes."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tests import sample_rules as R  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "sample_reference.json")))
F = np.float32


# ---------------------------------------------------------------------------------------------- 1. the rules
@pytest.mark.parametrize("case", GOLDEN["grid_sample"], ids=lambda c: c["name"])
def test_rules_match_reference_literals(case):
    got = R.grid_sample(np.array(case["input"], F), np.array(case["grid"], F), case["align_corners"])
    want = np.array(case["expected"], F)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-4  # expect_eq_1e4


@pytest.mark.parametrize("x_shape,grid_shape", [((2, 3, 5, 7), (2, 4, 6, 2)), ((2, 3, 1, 1), (2, 4, 6, 2)), ((2, 3, 1, 2), (2, 4, 6, 2)), ((2, 3, 2, 1), (2, 4, 6, 2))])
@pytest.mark.parametrize("align_corners", [False, True])
def test_rules_match_torch_grid_sample(x_shape, grid_shape, align_corners):
    import torch
    rng = np.random.default_rng(5)
    x = rng.standard_normal(x_shape).astype(F)
    grid = rng.uniform(-1.3, 1.3, grid_shape).astype(F)
    want = torch.nn.functional.grid_sample(torch.from_numpy(x), torch.from_numpy(grid), mode="bilinear", padding_mode="zeros", align_corners=align_corners).numpy()
    assert np.abs(R.grid_sample(x, grid, align_corners) - want).max() <= 1e-4


def test_rules_cast_and_special_coordinates():
    assert R.rust_f32_as_i32(np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, 2147483520.0, -2.5, 2.5, -0.0], F)).tolist() == \
        [0, R.I32_MAX, R.I32_MIN, R.I32_MAX, R.I32_MIN, 2147483520, -2, 2, 0]
    x = np.arange(1, 5, dtype=F).reshape(1, 1, 2, 2)
    g = np.array([[[[np.nan, 0], [np.inf, 0], [-np.inf, 0], [1e30, 0], [-1e30, 0], [2, 0], [-2, 0], [-0.0, -0.0]]]], F)
    y = R.grid_sample(x, g)[0, 0, 0]
    # NaN: index 0 with a NaN weight; +-Inf: the weight is Inf - Inf = NaN and 0 + (0 - 0) * NaN = NaN; +-1e30, +-2: far outside, weight finite, +0.0
    assert np.isnan(y[:3]).all() and (y[3:7] == 0).all() and not np.signbit(y[3:7]).any() and y[7] == 2.5
    # an empty input plane: zeros
    assert np.array_equal(R.grid_sample(np.zeros((1, 2, 0, 3), F), np.zeros((1, 2, 2, 2), F)), np.zeros((1, 2, 2, 2), F))
    # a zero-weight neighbour still contributes: at an exact pixel centre the right and lower neighbours' NaN reaches the output
    xn = x.copy()
    xn[0, 0, 1, 1] = np.nan
    centre = np.array([[[[-0.5, -0.5]]]], F)  # pixel (0, 0) of a 2x2 plane without align_corners: both weights are 0
    assert R.grid_sample(x, centre)[0, 0, 0, 0] == 1 and np.isnan(R.grid_sample(xn, centre)[0, 0, 0, 0])
    assert R.footprint(centre, 2, 2)[0, 0, 0].all()


def test_depth_to_space_rules():
    import torch
    for case in GOLDEN["depth_to_space"]:
        if "expected" in case:
            assert np.array_equal(R.depth_to_space(np.array(case["input"], F), case["block_size"], case["mode"]), np.array(case["expected"], F))
    rng = np.random.default_rng(6)
    for shape, b in (((2, 8, 3, 5), 2), ((1, 18, 2, 3), 3), ((3, 4, 1, 1), 2), ((2, 5, 3, 2), 1)):
        x = rng.standard_normal(shape).astype(F)
        n, c, h, w = shape
        assert np.array_equal(R.depth_to_space(x, b, "CRD"), torch.pixel_shuffle(torch.from_numpy(x), b).numpy())
        # the ONNX specification's DCR: reshape [n, b, b, c / b^2, h, w], transpose [0, 3, 4, 1, 5, 2], reshape
        spec = np.transpose(x.reshape(n, b, b, c // (b * b), h, w), [0, 3, 4, 1, 5, 2]).reshape(n, c // (b * b), h * b, w * b)
        assert np.array_equal(R.depth_to_space(x, b, "DCR"), spec)


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
    return e.value.kind, e.value.msg


def test_python_operators_on_a_recording_context():
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    ctx = _recording()
    t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
    x, grid = t(2, 3, 5, 7), t(2, 4, 6, 2)
    for align in (False, True):
        del ctx.calls[:]
        y = ops.GridSample(align_corners=align).run(ctx, [x, grid])[0]
        assert y.shape == (2, 3, 4, 6) and y.dtype == F and len(ctx.calls) == 1
        name, args = ctx.calls[0]
        assert name == "rten_hip_grid_sample_f32" and list(args[:7]) == [int(align), 2, 3, 5, 7, 4, 6]
        assert [a.value for a in args[7:]] == [x.ptr, grid.ptr, y.ptr]
    del ctx.calls[:]
    assert ops.GridSample().run(ctx, [t(2, 3, 5, 7), t(2, 0, 6, 2)])[0].shape == (2, 3, 0, 6) and ctx.calls == []  # an empty output launches nothing
    y = ops.GridSample().run(ctx, [t(2, 3, 0, 7), t(2, 1, 1, 2)])[0]
    assert y.shape == (2, 3, 1, 1) and [c[0] for c in ctx.calls] == ["rten_hip_grid_sample_f32"]  # an empty input plane: the entry point zero-fills
    assert ops.GridSample().align_corners is False and ops.GridSample().max_inputs() == 2

    for mode, view, perm in (("DCR", (2, 2, 2, 3, 5, 7), (0, 3, 4, 1, 5, 2)), ("CRD", (2, 3, 2, 2, 5, 7), (0, 1, 4, 2, 5, 3))):
        del ctx.calls[:]
        x = t(2, 12, 5, 7)
        y = ops.DepthToSpace(2, mode).run(ctx, [x])[0]
        assert y.shape == (2, 3, 10, 14) and len(ctx.calls) == 1  # ONE launch
        name, args = ctx.calls[0]
        assert name == "rten_hip_transpose_b32" and args[0] == 6 and tuple(args[1]) == view and tuple(args[2]) == perm
        assert isinstance(args[1], C.Array) and args[1]._type_ is C.c_int64 and args[2]._type_ is C.c_int32
        assert [a.value for a in args[3:]] == [x.ptr, y.ptr]
    del ctx.calls[:]
    assert ops.DepthToSpace(3).run(ctx, [t(0, 9, 2, 2)])[0].shape == (0, 1, 6, 6) and ctx.calls == []
    assert ops.DepthToSpace(2).mode == "DCR" and ops.DepthToSpace(2).max_inputs() == 1

    reg = ops.OpRegistry.with_all_ops()
    assert reg.get("GridSample") is ops.GridSample and reg.get("DepthToSpace") is ops.DepthToSpace


def test_python_operator_errors():
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    ctx = _recording()
    t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
    for case in GOLDEN["grid_sample_invalid"]:
        assert list(_refusal(ops.GridSample(), [t(*case["input_shape"]), t(*case["grid_shape"])])) == case["error"]
    for case in GOLDEN["depth_to_space"]:
        if "error" in case:
            mode = case["mode"]
            assert list(_refusal(ops.DepthToSpace(case["block_size"], mode), [t(*case["input_shape"])])) == case["error"]
    assert _refusal(ops.DepthToSpace(-1), [t(1, 4, 2, 2)]) == ("InvalidValue", "`block_size` must be > 0")
    with pytest.raises(ops.OpError) as e:  # the mode is one of the reference's two enum variants: refused at construction ...
        ops.DepthToSpace(2, "XYZ")
    assert (e.value.kind, e.value.msg) == ("UnsupportedValue", "DepthToSpace mode must be DCR or CRD")
    late = ops.DepthToSpace(2)
    late.mode = "crd"  # ... and, set afterwards, before anything is launched
    assert _refusal(late, [t(1, 4, 2, 2)]) == ("UnsupportedValue", "DepthToSpace mode must be DCR or CRD")
    # rank and type: as the other 4-D float32 operators
    assert _refusal(ops.DepthToSpace(2), [t(4, 2, 2)]) == ("InvalidValue", "input must have 4 dims (NCHW)")
    assert _refusal(ops.GridSample(), [t(3, 5, 7), t(1, 4, 6, 2)]) == ("InvalidValue", "input must have 4 dims (NCHW)")
    assert _refusal(ops.GridSample(), [t(1, 3, 5, 7), t(4, 6, 2)])[0] == "InvalidValue"
    assert _refusal(ops.GridSample(), [t(1, 3, 5, 7, dtype=np.int32), t(1, 4, 6, 2)])[0] == "InputCastFailed"
    assert _refusal(ops.GridSample(), [t(1, 3, 5, 7), t(1, 4, 6, 2, dtype=np.int32)])[0] == "InputCastFailed"
    assert _refusal(ops.DepthToSpace(2), [t(1, 4, 2, 2, dtype=np.int32)])[0] == "InputCastFailed"
    assert _refusal(ops.GridSample(), [t(1, 3, 5, 7)])[0] == "MissingInputs" and _refusal(ops.DepthToSpace(2), [])[0] == "MissingInputs"


# ---------------------------------------------------------------------------------------------- 3. the loader's checks, through the CLI
def _parse_only(tmp_path, name, data):
    from tests.test_graph_executor import run_cli
    p = tmp_path / name
    p.write_bytes(data)
    return run_cli("--parse-only", str(p))


def test_cli_parses_warp_and_subpixel_graphs(tmp_path):
    """Fails on a tree without the two operators: its --parse-only knows neither node (no `sample step` / `layout step` line), and its loader refuses
    each graph at that node ("operator GridSample is not available on the HIP backend")."""
    from rten_amd import onnx_writer as ow
    import torch_export as te
    for align in (False, True):
        out = _parse_only(tmp_path, "warp.onnx", ow.flow_warp_graph(align_corners=align)[0])
        assert out.returncode == 0, out.stderr
        assert "GridSample x1" in out.stdout and f'sample step GridSample "warp": bilinear, zero padding, align_corners {int(align)}' in out.stdout, out.stdout
        out = _parse_only(tmp_path, "warp_torch.onnx", te.warp_onnx(align_corners=align))
        assert out.returncode == 0, out.stderr
        assert "producer pytorch" in out.stdout and "GridSample x1" in out.stdout and f"zero padding, align_corners {int(align)}" in out.stdout, out.stdout
        assert "input  x: f32 [batch, 3, 6, 8]" in out.stdout
    for mode in ("DCR", "CRD"):
        out = _parse_only(tmp_path, "sr.onnx", ow.subpixel_sr_graph(mode)[0])
        assert out.returncode == 0, out.stderr
        assert "DepthToSpace x1" in out.stdout and f'layout step DepthToSpace "shuffle": mode {mode}, blocksize 2' in out.stdout, out.stdout
    # nn.PixelShuffle is Reshape / Transpose / Reshape in PyTorch's export: no DepthToSpace node
    out = _parse_only(tmp_path, "sr_torch.onnx", te.pixel_shuffle_sr_onnx(ow.subpixel_sr_graph("CRD")[1]))
    assert out.returncode == 0 and "DepthToSpace" not in out.stdout and "Transpose x1" in out.stdout and "Reshape x2" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("attrs,words", [({"mode": "nearest"}, ('GridSample warp', 'mode="nearest"')), ({"mode": "bicubic"}, ('GridSample warp', 'mode="bicubic"')),
                                         ({"mode": "cubic"}, ('GridSample warp', 'mode="cubic"')), ({"padding_mode": "border"}, ('GridSample warp', 'padding_mode="border"')),
                                         ({"padding_mode": "reflection"}, ('GridSample warp', 'padding_mode="reflection"'))])
def test_cli_refuses_grid_sample_attributes_by_node_name(tmp_path, attrs, words):
    from rten_amd import onnx_writer as ow
    out = _parse_only(tmp_path, "bad.onnx", ow.flow_warp_graph(**attrs)[0])
    assert out.returncode == 1 and all(w in out.stderr for w in words), out.stdout + out.stderr


def test_cli_reads_attribute_defaults_and_refuses_depth_to_space_modes(tmp_path):
    from rten_amd import onnx_writer as ow
    out = _parse_only(tmp_path, "bad.onnx", ow.subpixel_sr_graph("XYZ")[0])
    assert out.returncode == 1 and "DepthToSpace shuffle" in out.stderr and 'mode="XYZ"' in out.stderr, out.stdout + out.stderr
    x, y = [ow.value_info("x", ow.FLOAT, [1, 8, 2, 2])], [ow.value_info("y", ow.FLOAT, [1, 2, 4, 4])]
    out = _parse_only(tmp_path, "noblock.onnx", ow.model([ow.node("DepthToSpace", ["x"], ["y"], name="d2s")], x, y, []))
    assert out.returncode == 1 and "DepthToSpace d2s" in out.stderr and "blocksize" in out.stderr, out.stdout + out.stderr
    out = _parse_only(tmp_path, "negblock.onnx", ow.model([ow.node("DepthToSpace", ["x"], ["y"], name="d2s", blocksize=-2)], x, y, []))
    assert out.returncode == 1 and "DepthToSpace d2s" in out.stderr and "blocksize -2" in out.stderr, out.stdout + out.stderr
    out = _parse_only(tmp_path, "default.onnx", ow.model([ow.node("DepthToSpace", ["x"], ["y"], name="d2s", blocksize=2)], x, y, []))
    assert out.returncode == 0 and 'layout step DepthToSpace "d2s": mode DCR, blocksize 2' in out.stdout, out.stdout + out.stderr  # mode defaults to DCR
    # GridSample: the attribute cases of the reference's test_read_grid_sample_mode; align_corners defaults to 0
    gx = [ow.value_info("x", ow.FLOAT, [1, 1, 2, 2]), ow.value_info("g", ow.FLOAT, [1, 1, 1, 2])]
    gy = [ow.value_info("y", ow.FLOAT, [1, 1, 1, 1])]
    for case in GOLDEN["grid_sample_mode_attribute"]:
        attrs = {} if case["mode"] is None else {"mode": case["mode"]}
        out = _parse_only(tmp_path, "gs.onnx", ow.model([ow.node("GridSample", ["x", "g"], ["y"], name="gs", **attrs)], gx, gy, [], opset=20))
        if case["accepted"]:
            assert out.returncode == 0 and 'sample step GridSample "gs": bilinear, zero padding, align_corners 0' in out.stdout, out.stdout + out.stderr
        else:
            assert out.returncode == 1 and "GridSample gs" in out.stderr and f'mode="{case["mode"]}"' in out.stderr, out.stdout + out.stderr
