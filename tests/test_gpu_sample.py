"""GridSample and DepthToSpace on the device, bit for bit against tests/sample_rules.py: the raw entry point rten_hip_grid_sample_f32 (every launch
form of rten_amd/csrc/sample.hip, guarded operands and outputs, special coordinates, non-finite operands), both host layers (the Python operators
here, the C++ operators inside the graph executor), and the three graphs -- onnx_writer.flow_warp_graph, onnx_writer.subpixel_sr_graph and
tools/torch_export.warp_onnx -- node by node, fused, unfused, captured, on a clone, and one loaded model at changing shapes.

A tree without the two operators refuses each graph: "operator GridSample is not available on the HIP backend (no CPU fallback)"."""
import os
import sys

import numpy as np
import pytest

from tests import confine as K
from tests import sample_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32
pytestmark = pytest.mark.gpu

# sample.hip: a thread owns one output pixel (GS_THREADS = 256 per workgroup) and GS_CTILE_LARGE = 16, GS_CTILE_SMALL = 4 or 1 channels: the largest
# tile that leaves GS_MIN_BLOCKS = 1024 workgroups, i.e. 16 once pixel_blocks * ceil(C / 16) >= 1024, else 4 once pixel_blocks * ceil(C / 4) >= 1024.
# With one pixel block (batch 1, a plane of at most 256 pixels) the tile is 1 up to C = 4092, 4 from 4093 to 16368, 16 from 16369.
GS_THREADS, GS_CTILE_LARGE, GS_CTILE_SMALL, GS_MIN_BLOCKS = 256, 16, 4, 1024
PLANES = [(1, 1), (7, 9), (8, 8), (5, 13), (1, 257)]  # 1, 63, 64, 65, 257 output pixels: below / at / above a wave, two workgroups
TILE_CHANNELS = [4092, 4093, 4095, 4096, 4097, 16368, 16369, 16383, 16384, 16385]  # the last tile-1 and first tile-4 counts; one below / at / above a multiple of 4
#                                                                                    in tile 4; the last tile-4 and first tile-16 counts; the same around 16 in tile 16


def tile_of(channels, pixel_blocks):
    for t in (GS_CTILE_LARGE, GS_CTILE_SMALL):
        if pixel_blocks * -(-channels // t) >= GS_MIN_BLOCKS:
            return t
    return 1


def same_bits(got, want, what):
    """K.bits_equal (NaNs coincide, everything else equal) and, beyond it, the same sign on every zero."""
    K.bits_equal(got, want, what)
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), f"{what}: a zero's sign differs"


def sample(ctx, x, grid, align, leads=(0, 0, 0), what="", x_guards=(K.GUARD_FLAT, K.GUARD_FLAT)):
    """rten_hip_grid_sample_f32 on guarded x / grid / y, each `lead` elements off a 16-byte boundary: -> y, after checking that nothing but y was written."""
    n, c, in_h, in_w = x.shape
    _, out_h, out_w, _ = grid.shape
    xg, gg = K.Guarded(ctx, x, lead=leads[0], front=x_guards[0], back=x_guards[1]), K.Guarded(ctx, grid, lead=leads[1])
    shape = (n, c, out_h, out_w)
    out = K.Guarded(ctx, int(np.prod(shape)) * 4, lead=leads[2], front=K.nchw_guard(out_h * out_w), back=K.nchw_guard(out_h * out_w))
    ctx.call("rten_hip_grid_sample_f32", int(align), n, c, in_h, in_w, out_h, out_w, xg.vp, gg.vp, out.vp)
    ctx.sync()
    return out.check(out.raw(), shape, K.dense(shape), F, f"grid_sample {what} x {x.shape} grid {grid.shape} align {align} leads {leads}")


def check(ctx, x, grid, align, leads=(0, 0, 0), what="", x_guards=(K.GUARD_FLAT, K.GUARD_FLAT)):
    got = sample(ctx, x, grid, align, leads, what, x_guards)
    same_bits(got, R.grid_sample(x, grid, align), f"grid_sample {what} x {x.shape} grid {grid.shape} align {align} leads {leads}")
    return got


def operands(x_shape, out_hw, seed, spread=1.3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(x_shape).astype(F)
    return x, rng.uniform(-spread, spread, (x_shape[0],) + tuple(out_hw) + (2,)).astype(F)  # (some samples fall outside the plane)


# ================================================================================================ launch forms
@pytest.mark.parametrize("out_hw", PLANES)
@pytest.mark.parametrize("align", [False, True])
def test_planes_channels_and_batch_rows(ctx, out_hw, align):
    for channels in (1, 3):
        x, grid = operands((2, channels, 5, 7), out_hw, 100 + channels)
        got = check(ctx, x, grid, align)
        if out_hw != (1, 1):
            assert not np.array_equal(got[0], got[1])  # the two batch rows are distinct


@pytest.mark.parametrize("channels", TILE_CHANNELS + [70000])
def test_every_channel_tile(ctx, channels):
    """One pixel block; the channel count selects the tile (tile_of mirrors pick_ctile), ragged last tiles included."""
    want_tile = 1 if channels <= 4092 else 4 if channels <= 16368 else 16
    assert tile_of(channels, 1) == want_tile
    out_hw = (1, 1) if channels == 70000 else (5, 13)
    x, grid = operands((1, channels, 1, 1) if channels == 70000 else (1, channels, 2, 2), out_hw, channels, spread=1.0)
    check(ctx, x, grid, channels % 2 == 0, what=f"tile {want_tile}")


def test_more_channel_tiles_than_the_grid_cap_and_several_pixel_blocks(ctx):
    # 65537 tiles of 16 channels on a grid dimension capped at 65535: the stride loop's second trip
    channels = 16 * 65536 + 1
    assert tile_of(channels, 1) == 16 and -(-channels // 16) > 65535
    x, grid = operands((1, channels, 1, 1), (1, 1), 7, spread=0.5)
    check(ctx, x, grid, False, what="past the channel-tile grid cap")
    # three batch rows of two pixel blocks, tile 16 reached through the pixel blocks as well: 6 * ceil(2731 / 16) = 1026
    assert tile_of(2731, 6) == 16 and tile_of(2720, 6) == 4
    for channels in (2731, 2720):
        x, grid = operands((3, channels, 3, 2), (3, 100), channels)
        check(ctx, x, grid, True, what="several pixel blocks")


@pytest.mark.parametrize("leads", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 1, 3), (2, 2, 2)])
def test_misaligned_operands(ctx, leads):
    """x, grid and y 4, 8 and 12 bytes off a 16-byte boundary: the grid's pair is one 8-byte load only when its pointer allows it."""
    for out_hw in ((5, 13), (1, 257)):
        x, grid = operands((2, 3, 4, 6), out_hw, 31)
        check(ctx, x, grid, False, leads)


@pytest.mark.parametrize("in_hw", [(1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (5, 1)])
@pytest.mark.parametrize("align", [False, True])
def test_small_input_planes(ctx, in_hw, align):
    x, grid = operands((2, 3) + in_hw, (5, 13), 41)
    check(ctx, x, grid, align)


def test_empty_planes_and_bad_sizes(ctx):
    from rten_amd import lib as L
    for in_hw in ((0, 3), (3, 0), (0, 0)):  # an empty input plane: all zeros, and only y is written
        got = sample(ctx, np.zeros((2, 3) + in_hw, F), operands((2, 1, 1, 1), (5, 13), 1)[1], False)
        assert got.shape == (2, 3, 5, 13) and not got.view(np.uint32).any()
    for shape in ((2, 3, 0, 4), (2, 3, 4, 0), (0, 3, 4, 4), (2, 0, 4, 4)):  # an empty output: nothing is written
        n, c, oh, ow = shape
        out, xg, gg = K.Guarded(ctx, 64), K.Guarded(ctx, np.ones((max(n, 1), max(c, 1), 2, 2), F)), K.Guarded(ctx, np.zeros(64, F))
        ctx.call("rten_hip_grid_sample_f32", 0, n, c, 2, 2, oh, ow, xg.vp, gg.vp, out.vp)
        ctx.sync()
        assert (out.raw() == K.FILL).all(), shape
    buf = K.Guarded(ctx, np.zeros(64, F))
    for sizes in ((-1, 1, 1, 1, 1, 1), (1, -1, 1, 1, 1, 1), (1, 1, -1, 1, 1, 1), (1, 1, 1, -1, 1, 1), (1, 1, 1, 1, -1, 1), (1, 1, 1, 1, 1, -1)):
        with pytest.raises(L.HipError, match="grid_sample: bad dimension"):
            ctx.call("rten_hip_grid_sample_f32", 0, *sizes, buf.vp, buf.vp, buf.vp)


# ================================================================================================ coordinates
def special_values():
    one, none = F(1), F(-1)
    v = [none, np.nextafter(none, F(-2)), np.nextafter(none, F(0)), one, np.nextafter(one, F(2)), np.nextafter(one, F(0)),
         2, -2, 1e30, -1e30, np.inf, -np.inf, np.nan, -0.0, 0.0, 0.5, -0.5, 1 / 3, -3 / 7]
    return np.array(v, F)


@pytest.mark.parametrize("in_hw", [(5, 7), (2, 2), (1, 1), (1, 2), (2, 1), (4, 4)])
@pytest.mark.parametrize("align", [False, True])
def test_special_coordinates_and_pixel_centres(ctx, in_hw, align):
    """-1 and 1 and one ulp either side, +-2, +-1e30, +-Inf, NaN, -0.0 in every (x, y) combination; then the identity grid: exact pixel centres, where
    the lerp weight is 0 (or one rounding away from it)."""
    from rten_amd import onnx_writer as ow
    v = special_values()
    gx, gy = np.meshgrid(v, v)
    grid = np.stack([gx, gy], -1)[None].astype(F)
    x = operands((1, 3) + in_hw, (1, 1), 51)[0]
    check(ctx, x, grid, align, what="special values")
    centres = ow.base_grid(in_hw[0], in_hw[1], align)
    got = check(ctx, x, centres, align, what="pixel centres")
    if in_hw == (4, 4) and not align:  # a power-of-two plane without align_corners: the centres are exact, every weight is 0 and the sample IS the pixel
        assert np.array_equal(got, x)
    # ... and with a NaN as every right / lower neighbour's value the zero weight still lets it through (the rules say where)
    xn = x.copy()
    xn[..., -1, -1] = np.nan
    check(ctx, xn, centres, align, what="pixel centres, NaN corner")


def border_values(length):
    """Coordinates whose taps straddle and leave the plane along an axis of `length` pixels without align_corners (s = length * (g + 1) / 2 - 0.5):
    taps (-1, 0), (length - 1, length), (-2, -1), (length, length + 1), far outside, and both ends of the i32 range (and NaN: index 0)."""
    step = 2.0 / length
    return np.array([-1, 1, -1 - step, 1 + step, -1 - 3 * step, 1 + 3 * step, 0.0, 5e9, -5e9, 1e30, -1e30, np.inf, -np.inf, np.nan], F)


@pytest.mark.parametrize("x_guards,what", [((0, K.GUARD_FLAT), "x at the very start of its allocation"), ((K.GUARD_FLAT, 0), "x at the very end of its allocation")])
@pytest.mark.parametrize("in_hw", [(4, 4), (3, 5), (1, 1)])
def test_out_of_bounds_taps_with_x_at_an_end_of_its_allocation(ctx, x_guards, what, in_hw):
    """No guard in front of x (its first byte is the allocation's first), then none behind it: taps at (-1, -1), (-1, in_w), (in_h, -1), (in_h, in_w), one
    and several pixels further out and saturated at i32::MIN / i32::MAX, in every (x, y) combination, both align_corners values; two batch rows and five
    channels, so that the first and the last plane of x are both sampled.  The results are the rules' bits."""
    in_h, in_w = in_hw
    gx, gy = np.meshgrid(border_values(in_w), border_values(in_h))
    grid = np.ascontiguousarray(np.broadcast_to(np.stack([gx, gy], -1)[None], (2,) + gx.shape + (2,))).astype(F)
    x = operands((2, 5, in_h, in_w), (1, 1), 55)[0]
    if not x_guards[0]:
        ix0, ix1, _ = R._axis(grid[0, 0, :, 0], in_w, False)
        iy0, iy1, _ = R._axis(grid[0, :, 0, 1], in_h, False)
        assert {-2, -1, 0, in_w - 1, in_w, in_w + 1, R.I32_MIN, R.I32_MAX} <= set(ix0.tolist()) | set(ix1.tolist())  # the taps the coordinates are there for
        assert {-2, -1, 0, in_h - 1, in_h, in_h + 1, R.I32_MIN, R.I32_MAX} <= set(iy0.tolist()) | set(iy1.tolist())
    for align in (False, True):
        check(ctx, x, grid, align, what=what, x_guards=x_guards)


def test_null_pointers_are_refused_with_a_message(ctx):
    from rten_amd import lib as L
    buf = K.Guarded(ctx, np.zeros(64, F))
    for ptrs, match in (((buf.vp, buf.vp, None), "grid_sample: null output"), ((None, buf.vp, buf.vp), "grid_sample: null input or grid"),
                        ((buf.vp, None, buf.vp), "grid_sample: null input or grid")):
        with pytest.raises(L.HipError, match=match):
            ctx.call("rten_hip_grid_sample_f32", 0, 1, 1, 2, 2, 1, 1, *ptrs)
    ctx.call("rten_hip_grid_sample_f32", 0, 1, 1, 0, 2, 1, 1, None, None, buf.vp)  # an empty input plane needs neither x nor the grid
    ctx.sync()


# ================================================================================================ non-finite operands stay where the rules put them
@pytest.mark.parametrize("align", [False, True])
def test_a_nan_coordinate_changes_its_pixel_only(ctx, align):
    x, grid = operands((2, 5, 4, 6), (5, 13), 61, spread=0.9)
    clean = check(ctx, x, grid, align)
    for bad in (np.nan, np.inf):
        dirty_grid = grid.copy()
        dirty_grid[1, 2, 7, 0] = bad
        dirty = check(ctx, x, dirty_grid, align)
        changed = clean.view(np.uint32) != dirty.view(np.uint32)
        want = np.zeros_like(changed)
        want[1, :, 2, 7] = True
        assert np.array_equal(changed, want) and np.isnan(dirty[1, :, 2, 7]).all()


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_pixel_reaches_exactly_its_footprint(ctx, align, bad):
    """The outputs that change are those of the pixel's (batch row, channel) whose 2x2 neighbourhood holds it -- zero-weight neighbours included (the
    identity grid's rows put the pixel there with weight 0)."""
    from rten_amd import onnx_writer as ow
    x, grid = operands((2, 3, 4, 4), (6, 11), 71, spread=1.1)
    grid[0, :4, :4] = ow.base_grid(4, 4, align)[0]  # exact centres: (iy, ix) = the pixel itself, both weights 0
    clean = check(ctx, x, grid, align)
    hit = R.footprint(grid, 4, 4, align)
    for (n, c, iy, ix) in ((0, 1, 2, 3), (1, 2, 0, 0), (0, 0, 3, 3)):
        dirty_x = x.copy()
        dirty_x[n, c, iy, ix] = bad
        dirty = check(ctx, dirty_x, grid, align)
        want = np.zeros(clean.shape, bool)
        want[n, c] = hit[n, :, :, iy, ix]
        assert want.any() and np.array_equal(~np.isfinite(dirty), want), (n, c, iy, ix)  # (an Inf under a non-zero weight stays an Inf)
        assert np.array_equal(dirty[~want].view(np.uint32), clean[~want].view(np.uint32))


# ================================================================================================ the Python host layer
def dev(ctx, a):
    from rten_amd.tensor import DeviceTensor
    return DeviceTensor.from_numpy(ctx, np.ascontiguousarray(a))


def test_python_operators_on_the_device(ctx):
    from rten_amd import ops
    for align in (False, True):
        x, grid = operands((2, 3, 5, 7), (4, 6), 81)
        same_bits(ops.GridSample(align).run(ctx, [dev(ctx, x), dev(ctx, grid)])[0].numpy(), R.grid_sample(x, grid, align), f"GridSample align {align}")
    y = ops.GridSample().run(ctx, [dev(ctx, np.zeros((2, 3, 0, 7), F)), dev(ctx, np.zeros((2, 4, 6, 2), F))])[0]
    assert y.shape == (2, 3, 4, 6) and not y.numpy().any()
    rng = np.random.default_rng(82)
    for shape, b in (((2, 12, 5, 7), 2), ((1, 18, 3, 2), 3), ((3, 4, 1, 1), 2), ((2, 3, 4, 5), 1), ((1, 8, 33, 65), 2)):
        x = rng.standard_normal(shape).astype(F)
        for mode in ("DCR", "CRD"):
            got = ops.DepthToSpace(b, mode).run(ctx, [dev(ctx, x)])[0].numpy()
            assert np.array_equal(got.view(np.uint32), R.depth_to_space(x, b, mode).view(np.uint32)), (shape, b, mode)


# ================================================================================================ graphs
CLI_MODES = (("-t",), (), ("--no-fuse",), ("--graph", "-n", "2"))  # node by node (a sync after every step), fused, unfused, captured and replayed


def run_cli_graph(tmp_path, data, inputs, outputs, sizes, extra):
    from tests.test_graph_executor import run_cli
    path = tmp_path / "model.onnx"
    path.write_bytes(data)
    args = list(extra)
    for k, v in sizes.items():
        args += ["-s", f"{k}={v}"]
    for name, arr in inputs.items():
        arr.tofile(tmp_path / (name + ".bin"))
        args += ["--input", f"{name}={tmp_path / (name + '.bin')}"]
    for name in outputs:
        args += ["--dump", f"{name}={tmp_path / (name + '.out')}"]
    r = run_cli(*args, str(path))
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2500:]
    return {name: np.fromfile(tmp_path / (name + ".out"), F) for name in outputs}, r.stdout


def model_run(ctx, m, feeds):
    """One bind / prepare (capture) / run of a rten_amd.lib.Model: -> its first output."""
    from rten_amd.tensor import DeviceTensor
    for name in m.inputs:
        a = feeds[name]
        DeviceTensor(ctx, a.shape, a.dtype, ptr=m.bind_input(name, a.shape), keepalive=m).upload(a)
    ctx.sync()
    m.prepare()
    m.run()
    m.sync()
    ptr, shape = m.output(0)
    return DeviceTensor(ctx, shape, F, ptr=ptr, keepalive=m).numpy()


# One process: load, six runs and a capture of a graph of a few nodes.  Start-up and code-object loading dominate; tests/test_gpu_graph_sessions.py measured 0.41 s
# for its slowest process and allows 5 s, tests/test_gpu_graph_fuzz.py 6 s; four times the former, for a cold code-object cache on a shared machine.
SESSION_TIMEOUT_S = 20.0


def through_one_graph(ctx, tmp_path, data, bindings):
    """`bindings` = [(feeds, expected)] of at least two shapes, the last repeating the first shape with other values.
    ONE loaded Graph in one process of tests/cpp/graph_session.cpp: an eager run at every binding, a capture at the first, a replay, the last binding's
    values written into the captured feeds and replayed, an eager run at the second shape again -- no reload in between.  Then the executor behind the
    C ABI (rten_amd.lib.Model: fused, captured by prepare) at the first binding and a clone of it on a second context at the last."""
    import subprocess
    from safetensors.numpy import save_file
    from rten_amd import lib as L
    from tests import graph_sessions as gs
    from tests.test_gpu_graph_fuzz import read_safetensors
    assert [a.shape for a in bindings[0][0].values()] == [a.shape for a in bindings[-1][0].values()]
    d = str(tmp_path)
    open(os.path.join(d, "session.onnx"), "wb").write(data)
    for k, (feeds, _) in enumerate(bindings):
        save_file({nm: np.ascontiguousarray(a) for nm, a in feeds.items()}, os.path.join(d, f"b{k}.safetensors"))
    last = len(bindings) - 1
    actions = [("run", k, k) for k in range(len(bindings))] + [("capture", 0, 0), ("replay", None, 0), ("refill", last, None), ("replay", None, last), ("run", 1, 1)]
    lines, outputs = [], []
    for i, (verb, src, binding) in enumerate(actions):
        words = [verb] + ([os.path.join(d, f"b{src}.safetensors")] if src is not None else [])
        if binding is not None:
            outputs.append((os.path.join(d, f"out{i}.safetensors"), binding, verb))
            words.append(outputs[-1][0])
        lines.append(" ".join(words))
    open(os.path.join(d, "script.txt"), "w").write("\n".join(lines) + "\n")
    r = subprocess.run([gs.build_session_probe(), os.path.join(d, "session.onnx"), os.path.join(d, "script.txt")], capture_output=True, text=True, timeout=SESSION_TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    for path, binding, verb in outputs:
        (_, got), = read_safetensors(path)
        same_bits(got, bindings[binding][1], f"one graph, {verb} at binding {binding}")
    m = L.Model(ctx, data)
    other = L.Context(0)
    try:
        same_bits(model_run(ctx, m, bindings[0][0]), bindings[0][1], "the C-ABI model")
        lane = m.clone(other)
        try:
            same_bits(model_run(other, lane, bindings[last][0]), bindings[last][1], "its clone on a second context")
        finally:
            lane.close()
    finally:
        m.close()
        other.close()


def flow_warp_rules(w, x, flow, align):
    from oracle import ref
    feat = ref.conv2d_f32(x, w["feat"][0], w["feat"][1], pads=(1, 1, 1, 1))
    grid = (np.ascontiguousarray(flow.transpose(0, 2, 3, 1)) + w["base_grid"]).astype(F)
    return ref.conv2d_f32(R.grid_sample(feat, grid, align), w["out"][0], w["out"][1])


@pytest.mark.parametrize("align", [False, True])
def test_flow_warp_graph(ctx, tmp_path, align):
    from rten_amd import onnx_writer as ow
    data, w = ow.flow_warp_graph(align_corners=align)  # flow [batch, 2, 6, 9]; x's plane is free
    rng = np.random.default_rng(91)
    bindings = []
    for batch, h, w_ in ((2, 6, 9), (3, 4, 11), (2, 6, 9)):
        x = rng.standard_normal((batch, 3, h, w_)).astype(F)
        flow = rng.uniform(-0.6, 0.6, (batch, 2, 6, 9)).astype(F)
        bindings.append(({"x": x, "flow": flow}, flow_warp_rules(w, x, flow, align)))
    feeds, want = bindings[1]
    for extra in CLI_MODES:
        got, log = run_cli_graph(tmp_path, data, feeds, ["y"], {"batch": 3, "h": 4, "w": 11}, extra)
        same_bits(got["y"].reshape(want.shape), want, f"flow_warp {extra}")
        if extra == ("-t",):
            assert "GridSample" in log, log[-2500:]
    through_one_graph(ctx, tmp_path, data, bindings)


@pytest.mark.parametrize("mode", ["DCR", "CRD"])
def test_subpixel_sr_graph(ctx, tmp_path, mode):
    from oracle import ref
    from rten_amd import onnx_writer as ow
    import torch_export as te
    data, w = ow.subpixel_sr_graph(mode)
    rng = np.random.default_rng(92)

    def rules(x):
        a = ref.relu(ref.conv2d_f32(x, w["c1"][0], w["c1"][1], pads=(1, 1, 1, 1)))
        return R.depth_to_space(ref.conv2d_f32(a, w["c2"][0], w["c2"][1], pads=(1, 1, 1, 1)), 2, mode)
    bindings = []
    for shape in ((2, 3, 5, 7), (3, 3, 8, 4), (2, 3, 5, 7)):
        x = rng.standard_normal(shape).astype(F)
        bindings.append(({"x": x}, rules(x)))
    feeds, want = bindings[0]
    for extra in CLI_MODES:
        got, log = run_cli_graph(tmp_path, data, feeds, ["y"], {"batch": 2, "h": 5, "w": 7}, extra)
        same_bits(got["y"].reshape(want.shape), want, f"subpixel_sr {mode} {extra}")
        if extra == ("-t",):
            assert "DepthToSpace" in log, log[-2500:]
    through_one_graph(ctx, tmp_path, data, bindings)
    if mode == "CRD":  # the same network as PyTorch exports it with nn.PixelShuffle (Reshape / 6-D Transpose / Reshape), same weights: the same bits
        got, log = run_cli_graph(tmp_path, te.pixel_shuffle_sr_onnx(w, 2, 2, 5, 7), feeds, ["y"], {}, ())
        assert "DepthToSpace" not in log
        same_bits(got["y"].reshape(want.shape), want, "PixelShuffle export against DepthToSpace CRD")


@pytest.mark.parametrize("align", [False, True])
def test_torch_exported_warp(ctx, tmp_path, align):
    import torch
    from oracle import ref
    from rten_amd import onnx_writer as ow
    import torch_export as te
    module = te.warp_module(align_corners=align)
    data = te.warp_onnx(module, align_corners=align)  # x [batch, 3, 6, 8], grid [batch, 6, 8, 2]
    sd = {k: v.detach().numpy() for k, v in module.state_dict().items()}
    base = ow.base_grid(6, 8, align)
    rng = np.random.default_rng(93)

    def rules(x):
        f = ref.conv2d_f32(x, sd["feat.weight"], sd["feat.bias"], pads=(1, 1, 1, 1))
        flow = (ref.tanh(ref.conv2d_f32(f, sd["flow.weight"], sd["flow.bias"], pads=(1, 1, 1, 1))) * F(0.5)).astype(F)
        return R.grid_sample(f, (base + np.ascontiguousarray(flow.transpose(0, 2, 3, 1))).astype(F), align)
    bindings = []
    for batch in (2, 3, 2):
        x = (rng.standard_normal((batch, 3, 6, 8)) * 2).astype(F)
        bindings.append(({"x": x, "grid": np.ascontiguousarray(np.broadcast_to(base, (batch, 6, 8, 2)))}, rules(x)))
    feeds, want = bindings[1]
    for extra in CLI_MODES:
        got, _ = run_cli_graph(tmp_path, data, feeds, ["warped"], {"batch": 3}, extra)
        same_bits(got["warped"].reshape(want.shape), want, f"warp_onnx {extra}")
    through_one_graph(ctx, tmp_path, data, bindings)
    with torch.no_grad():
        t = module(torch.from_numpy(feeds["x"]), torch.from_numpy(feeds["grid"])).numpy()
    np.testing.assert_allclose(want, t, rtol=1e-4, atol=1e-4)
