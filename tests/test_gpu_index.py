"""CumSum, GatherElements, Trilu and Tile on the device, bit for bit against tests/index_rules.py: the raw entry points of rten_amd/csrc/scan.hip (both
CumSum forms around every geometry constant, guarded operands and outputs, edge values, clamped indices with x at either end of its allocation), the
Python operators, and the graphs -- onnx_writer.index_ops_graph (every attribute on device data), tools/torch_export.roberta_onnx and
causal_decoder_onnx -- node by node, fused, unfused, captured, on a clone, and one loaded dynamic model at two batch / sequence sizes in both orders.

A tree without the four operators refuses each graph: "operator CumSum is not available on the HIP backend (no CPU fallback)"."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import confine as K
from tests import index_rules as R
from tests.test_index_ops import SCAN_CHUNK, SCAN_MAX_BLOCKS, SCAN_ROWS, SCAN_THREADS, wide_range_lane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F, I = np.float32, np.int32
pytestmark = pytest.mark.gpu
DT = {np.dtype(F): 0, np.dtype(I): 1}
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def same_bits(got, want, what):
    """Same shape, dtype and bits, NaNs coinciding (any payload) and the sign of every zero included."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.dtype(F):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs differ"
        ok = ~nan
        bad = np.flatnonzero(got[ok].view(np.uint32) != want[ok].view(np.uint32))
        assert bad.size == 0, f"{what}: {bad.size} elements differ, first {got[ok][bad[0]]!r} instead of {want[ok][bad[0]]!r}"
    else:
        assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} elements differ"


def i64(v):
    import ctypes as C
    return (C.c_int64 * max(len(v), 1))(*[int(a) for a in v])


def operand(shape, dtype, seed):
    n = int(np.prod(shape))
    if np.dtype(dtype) == np.dtype(F):
        return wide_range_lane(n, seed).reshape(shape)
    return np.random.default_rng(seed).integers(-1000, 1000, shape).astype(I)


# ================================================================================================ CumSum
def cumsum(ctx, x, axis, exclusive=False, reverse=False, leads=(0, 0), what=""):
    """rten_hip_cumsum_b32 on guarded x / y, each `lead` elements off a 16-byte boundary -> y, after checking that nothing but y was written."""
    ax = axis % x.ndim
    outer, inner = int(np.prod(x.shape[:ax])), int(np.prod(x.shape[ax + 1:]))
    xg, out = K.Guarded(ctx, x, lead=leads[0]), K.Guarded(ctx, x.nbytes, lead=leads[1])
    ctx.call("rten_hip_cumsum_b32", DT[x.dtype], int(exclusive), int(reverse), outer, x.shape[ax], inner, xg.vp, out.vp)
    ctx.sync()
    what = f"cumsum {what} {x.dtype} {x.shape} axis {axis} exclusive {exclusive} reverse {reverse} leads {leads}"
    got = out.check(out.raw(), x.shape, K.dense(x.shape), x.dtype, what)
    same_bits(got, R.cum_sum(x, axis, exclusive, reverse), what)
    return got


MODES = [(False, False), (True, False), (False, True), (True, True)]
ROW_LENGTHS = sorted({1, 2, 63, 64, 65, SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 2 * SCAN_CHUNK + 1})
ROW_COUNTS = [1, SCAN_ROWS - 1, SCAN_ROWS, SCAN_ROWS + 1]


@pytest.mark.parametrize("dtype", [F, I])
@pytest.mark.parametrize("exclusive,reverse", MODES)
def test_cumsum_row_form(ctx, dtype, exclusive, reverse):
    """inner == 1: every axis length around the LDS chunk and every row count around the row block; wide-range f32 rows, on which a chunk-wise sum differs
    from the sequential one (tests/test_index_ops.py shows that on the CPU)."""
    for n in ROW_LENGTHS:
        for rows in ROW_COUNTS:
            cumsum(ctx, operand((rows, n), dtype, 1000 * rows + n), 1, exclusive, reverse, what="row form")


@pytest.mark.parametrize("leads", [(1, 0), (0, 1), (3, 2), (2, 3)])
@pytest.mark.parametrize("dtype", [F, I])
def test_cumsum_row_form_misaligned(ctx, dtype, leads):
    for exclusive, reverse in MODES:
        cumsum(ctx, operand((SCAN_ROWS + 1, 2 * SCAN_CHUNK + 1), dtype, 7), -1, exclusive, reverse, leads, "row form, off a 16-byte boundary")


def test_cumsum_row_form_more_row_blocks_than_the_grid_cap(ctx):
    rows = SCAN_ROWS * SCAN_MAX_BLOCKS + 3  # the row-block loop's second trip
    cumsum(ctx, operand((rows, 3), F, 8), 1, what="row form past the grid cap")


@pytest.mark.parametrize("dtype", [F, I])
@pytest.mark.parametrize("exclusive,reverse", MODES)
def test_cumsum_column_form(ctx, dtype, exclusive, reverse):
    """inner > 1: inner 3, 64, 65 at axis 0 and at a middle axis of a rank-4 tensor; a trailing axis of 1 makes inner 1, which the entry point gives to the row form."""
    for inner in (1, 3, 64, 65):
        cumsum(ctx, operand((7, 2, inner), dtype, inner), 0, exclusive, reverse, what=f"axis 0, inner {2 * inner}")
        cumsum(ctx, operand((2, 3, 67, inner), dtype, inner + 1), 2, exclusive, reverse, what=f"middle axis, inner {inner}")
        cumsum(ctx, operand((3, 130, inner), dtype, inner + 2), 1, exclusive, reverse, (1, 3), what=f"inner {inner}, misaligned")


def test_cumsum_column_form_more_lanes_than_the_grid_cap(ctx):
    lanes = SCAN_THREADS * SCAN_MAX_BLOCKS + 5
    cumsum(ctx, operand((2, lanes), F, 9), 0, what="column form past the grid cap")
    cumsum(ctx, operand((2, lanes), I, 9), 0, True, True, what="column form past the grid cap")


@pytest.mark.parametrize("form", ["row", "column"])
def test_cumsum_edge_values(ctx, form):
    def shaped(lane_major):  # [lanes, n] data as the form's operand: rows as they are, columns transposed (axis 0, inner = lanes)
        return (lane_major, 1) if form == "row" else (np.ascontiguousarray(lane_major.T), 0)
    n = 2 * SCAN_CHUNK + 1
    # a leading -0.0 (from either end): the first add is +0.0 + -0.0 = +0.0
    x = np.zeros((3, n), F)
    x[0, :3] = -0.0
    x[1, -2:] = -0.0
    x[2] = -0.0
    for exclusive, reverse in MODES:
        got = cumsum(ctx, *shaped(x), exclusive, reverse, what=f"{form}, -0.0")
        assert not np.signbit(got).any()
    # NaN, +Inf then -Inf in the middle of a lane stay in that lane and reach only what follows in walking order (K.rows_nonfinite: rows 1..3 of 5)
    for cols in K.ROWS_NONFINITE_COLS + [n]:
        base = operand((5, cols), F, cols)
        x, dep = K.rows_nonfinite(base)
        x[3, cols // 2] = np.inf  # row 3: +Inf in the middle, -Inf at the end: Inf - Inf = NaN in the last element only (forward)
        for exclusive, reverse in MODES:
            xs, axis = shaped(x)
            got = cumsum(ctx, xs, axis, exclusive, reverse, what=f"{form}, non-finite")
            lanes = got if form == "row" else got.T
            assert np.isfinite(lanes[~dep]).all() and np.array_equal(lanes[~dep].view(np.uint32), R.cum_sum(base, 1, exclusive, reverse)[~dep].view(np.uint32))
            mid = cols // 2
            if not exclusive:  # row 2 holds one +Inf at `mid`: before it in walking order the sums are finite, from it on they are +Inf
                before = lanes[2, mid + 1:] if reverse else lanes[2, :mid]
                after = lanes[2, :mid + 1] if reverse else lanes[2, mid:]
                assert np.isfinite(before).all() and (after == np.inf).all()
    # int32 lanes that pass INT32_MAX wrap
    x = np.full((3, n), I32_MAX // 50, I)
    x[1] = I32_MIN // 60
    x[2, ::2] = I32_MAX
    for exclusive, reverse in MODES:
        got = cumsum(ctx, *shaped(x), exclusive, reverse, what=f"{form}, int32 wrap")
        assert (got < 0).any() and (got > 0).any()


def test_cumsum_empty_and_bad_arguments(ctx):
    from rten_amd import lib as L
    buf, out = K.Guarded(ctx, np.ones(64, F)), K.Guarded(ctx, 256)
    for view in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 4, 1)):  # an empty tensor launches nothing
        ctx.call("rten_hip_cumsum_b32", 0, 0, 0, *view, buf.vp, out.vp)
    ctx.sync()
    assert (out.raw() == K.FILL).all()
    for args, match in (((2, 0, 0, 1, 4, 1), "cumsum: float32 or int32 only"), ((0, 0, 0, -1, 4, 1), "cumsum: bad dimension"), ((0, 0, 0, 1, 4, -1), "cumsum: bad dimension")):
        with pytest.raises(L.HipError, match=match):
            ctx.call("rten_hip_cumsum_b32", *args, buf.vp, out.vp)
    with pytest.raises(L.HipError, match="cumsum: null input or output"):
        ctx.call("rten_hip_cumsum_b32", 0, 0, 0, 1, 4, 1, None, out.vp)


# ================================================================================================ GatherElements
def gather_elements(ctx, x, ids, axis, clamp=False, x_guards=(K.GUARD_FLAT, K.GUARD_FLAT), what=""):
    ax = axis % x.ndim
    xg, ig = K.Guarded(ctx, x, front=x_guards[0], back=x_guards[1]), K.Guarded(ctx, ids, lead=1)
    out = K.Guarded(ctx, ids.size * 4, lead=3)
    ctx.call("rten_hip_gather_elements_b32", x.ndim, i64(x.shape), i64(ids.shape), ax, xg.vp, ig.vp, out.vp)
    ctx.sync()
    what = f"gather_elements {what} x {x.dtype} {x.shape} ids {ids.shape} axis {axis}"
    got = out.check(out.raw(), ids.shape, K.dense(ids.shape), x.dtype, what)
    same_bits(got, R.gather_elements(x, ids, axis, clamp=clamp), what)
    return got


@pytest.mark.parametrize("dtype", [F, I])
def test_gather_elements_axes_shapes_and_negative_indices(ctx, dtype):
    rng = np.random.default_rng(21)
    x = operand((5, 66, 7), dtype, 21)
    for axis in (0, 1, 2, -1, -3):
        alen = x.shape[axis]
        for ishape in ((5, 66, 7), (3, 64, 2), (1, 1, 1)):  # the data's extent, smaller on every dim, a single element
            ishape = tuple(9 if d == axis % 3 else s for d, s in enumerate(ishape))  # (the axis dim is free: longer than some axes, shorter than others)
            ids = rng.integers(-alen, alen, ishape).astype(I)  # negative indices add the axis length once
            gather_elements(ctx, x, ids, axis)
    x1 = operand((300,), dtype, 22)
    gather_elements(ctx, x1, rng.integers(-300, 300, (1000,)).astype(I), 0, what="rank 1")
    x6 = operand((2, 3, 2, 4, 3, 5), dtype, 23)
    for axis in (0, 3, 5):
        gather_elements(ctx, x6, rng.integers(-x6.shape[axis], x6.shape[axis], (2, 2, 2, 3, 3, 4)).astype(I), axis, what="rank 6")
    gather_elements(ctx, x, np.zeros((5, 0, 7), I), 1, what="empty indices")
    big = rng.integers(0, 3, (SCAN_THREADS * SCAN_MAX_BLOCKS + 9, 1)).astype(I)  # more outputs than the grid covers in one trip
    gather_elements(ctx, operand((big.shape[0], 3), dtype, 24), big, 1, what="past the grid cap")


@pytest.mark.parametrize("x_guards,where", [((0, K.GUARD_FLAT), "x at the very start of its allocation"), ((K.GUARD_FLAT, 0), "x at the very end of its allocation")])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gather_elements_clamps_out_of_range_indices_inside_x(ctx, x_guards, where, axis):
    """The deliberate deviation (the reference: "Entry in `indices` is out of range"): the index is normalised, then clamped to the axis, before the address is
    formed.  No guard in front of x, then none behind it: a read outside x would be outside the allocation.  The result is the clamped element."""
    x = operand((3, 4, 5), F, 31)
    alen = x.shape[axis]
    bad = np.array([alen, -alen - 1, I32_MAX, I32_MIN, alen + 7, -2 * alen, 0, -1, alen - 1, -alen], I)
    ishape = [3, 4, 5]
    ishape[axis] = bad.size
    ids = np.moveaxis(np.broadcast_to(bad, [s for d, s in enumerate(ishape) if d != axis] + [bad.size]), -1, axis)
    got = gather_elements(ctx, x, np.ascontiguousarray(ids), axis, clamp=True, x_guards=x_guards, what=where)
    lanes = np.moveaxis(got, axis, -1)
    first, last = np.moveaxis(x, axis, -1)[..., 0], np.moveaxis(x, axis, -1)[..., -1]
    assert np.array_equal(lanes[..., 0], last) and np.array_equal(lanes[..., 1], first) and np.array_equal(lanes[..., 2], last) and np.array_equal(lanes[..., 3], first)


def test_gather_elements_refusals(ctx):
    from rten_amd import lib as L
    buf = K.Guarded(ctx, np.zeros(64, I))
    for args, match in (((2, i64([2, 2]), i64([2, 3]), 0), "`indices` size must be <= input size in non-axis dimensions"), ((2, i64([2, 2]), i64([2, 2]), 2), "axis inside them"),
                        ((7, i64([1] * 7), i64([1] * 7), 0), "1 to 6 dims"), ((1, i64([0]), i64([2]), 0), "Entry in `indices` is out of range")):
        with pytest.raises(L.HipError, match=match):
            ctx.call("rten_hip_gather_elements_b32", *args, buf.vp, buf.vp, buf.vp)


# ================================================================================================ Trilu
@pytest.mark.parametrize("dtype", [F, I])
@pytest.mark.parametrize("upper", [True, False])
def test_trilu_shapes_and_diagonals(ctx, dtype, upper):
    for rows, cols in ((1, 1), (1, 5), (5, 1), (63, 65), (64, 64)):
        for batch in (1, 3):
            x = operand((batch, rows, cols), dtype, rows * cols + batch)
            xg = K.Guarded(ctx, x, lead=1)
            for k in (-65, -1, 0, 1, 65, I32_MAX, I32_MIN, 2 ** 31 + 5, -2 ** 31 - 5, 2 ** 40, -2 ** 40):
                out = K.Guarded(ctx, x.nbytes, lead=2)
                ctx.call("rten_hip_trilu_b32", int(upper), k, batch, rows, cols, xg.vp, out.vp)
                ctx.sync()
                what = f"trilu {x.dtype} {x.shape} k {k} upper {upper}"
                same_bits(out.check(out.raw(), x.shape, K.dense(x.shape), x.dtype, what), R.trilu(x, k, upper), what)


@pytest.mark.parametrize("upper", [True, False])
def test_trilu_masked_nans_never_reach_the_output(ctx, upper):
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    for k in (-3, 0, 2):
        x = operand((3, 63, 65), F, 41)
        kept = R.trilu(np.ones_like(x), k, upper) != 0
        x[~kept] = np.nan
        x[0][~kept[0]] = -np.inf
        got = ops.Trilu(upper).run(ctx, [DeviceTensor.from_numpy(ctx, x), np.array(k, I)])[0].numpy()
        same_bits(got, R.trilu(x, k, upper), f"trilu masked NaN k {k} upper {upper}")
        assert np.isfinite(got).all() and not got[~kept].view(np.uint32).any()  # the all-zero word: +0.0


def test_trilu_past_the_grid_cap_and_empty(ctx):
    x = operand((2, 800, 700), I, 42)  # more elements than the grid covers in one trip
    xg, out = K.Guarded(ctx, x), K.Guarded(ctx, x.nbytes)
    ctx.call("rten_hip_trilu_b32", 0, -100, 2, 800, 700, xg.vp, out.vp)
    ctx.sync()
    same_bits(out.check(out.raw(), x.shape, K.dense(x.shape), I, "trilu past the grid cap"), R.trilu(x, -100, False), "trilu past the grid cap")
    out = K.Guarded(ctx, 64)
    for view in ((0, 3, 3), (2, 0, 3), (2, 3, 0)):
        ctx.call("rten_hip_trilu_b32", 1, 0, *view, xg.vp, out.vp)
    ctx.sync()
    assert (out.raw() == K.FILL).all()


# ================================================================================================ Tile
def tile(ctx, x, repeats, what=""):
    oshape = tuple(s * r for s, r in zip(x.shape, repeats))
    xg, out = K.Guarded(ctx, x, lead=1), K.Guarded(ctx, max(int(np.prod(oshape)), 1) * 4, lead=3)
    ctx.call("rten_hip_tile_b32", x.ndim, i64(x.shape), i64(repeats), xg.vp, out.vp)
    ctx.sync()
    what = f"tile {what} {x.dtype} {x.shape} x {list(repeats)}"
    if 0 in oshape:
        assert (out.raw() == K.FILL).all(), what  # an empty output: nothing is launched, nothing written
        return
    same_bits(out.check(out.raw(), oshape, K.dense(oshape), x.dtype, what), R.tile(x, repeats), what)


@pytest.mark.parametrize("dtype", [F, I])
def test_tile_repeats(ctx, dtype):
    x = operand((3, 5, 7), dtype, 51)
    for repeats in ((1, 1, 1), (3, 1, 1), (1, 3, 1), (1, 1, 3), (0, 1, 3), (3, 0, 1), (1, 3, 0), (2, 3, 4), (3, 1, 0)):
        tile(ctx, x, repeats)
    tile(ctx, operand((70,), dtype, 52), (9,), "rank 1")
    tile(ctx, operand((1,), dtype, 52), (300,), "rank 1")
    tile(ctx, operand((2, 1, 3, 2, 1, 3), dtype, 53), (1, 4, 2, 1, 3, 2), "rank 6")
    tile(ctx, operand((1, 1, 2, 2, 2, 65), dtype, 54), (2, 2, 1, 1, 1, 1), "rank 6")
    tile(ctx, operand((3, 5), dtype, 55), (300, 250), "an output past the grid cap")
    assert 3 * 300 * 5 * 250 > SCAN_THREADS * SCAN_MAX_BLOCKS


def test_tile_refusals(ctx):
    from rten_amd import lib as L
    buf = K.Guarded(ctx, np.zeros(64, I))
    with pytest.raises(L.HipError, match="invalid repeats"):
        ctx.call("rten_hip_tile_b32", 2, i64([2, 2]), i64([1, -1]), buf.vp, buf.vp)
    with pytest.raises(L.HipError, match="tile: more than 6 dims"):
        ctx.call("rten_hip_tile_b32", 7, i64([1] * 7), i64([1] * 7), buf.vp, buf.vp)


# ================================================================================================ the Python host layer
def dev(ctx, a):
    from rten_amd.tensor import DeviceTensor
    return DeviceTensor.from_numpy(ctx, np.ascontiguousarray(a))


def test_python_operators_on_the_device(ctx):
    from rten_amd import ops
    rng = np.random.default_rng(61)
    for dtype in (F, I):
        x = operand((3, 70, 5), dtype, 61)
        for axis in (0, 1, 2, -1):
            for exclusive, reverse in MODES:
                same_bits(ops.CumSum(exclusive, reverse).run(ctx, [dev(ctx, x), np.array(axis, I)])[0].numpy(), R.cum_sum(x, axis, exclusive, reverse), f"CumSum axis {axis}")
        ids = rng.integers(-3, 3, (3, 9, 4)).astype(I)
        same_bits(ops.GatherElements(0).run(ctx, [dev(ctx, x), dev(ctx, ids)])[0].numpy(), R.gather_elements(x, ids, 0), "GatherElements, device indices")
        same_bits(ops.GatherElements(-3).run(ctx, [dev(ctx, x), ids])[0].numpy(), R.gather_elements(x, ids, 0), "GatherElements, host indices")
        same_bits(ops.Trilu(False).run(ctx, [dev(ctx, x), np.array(-2, I)])[0].numpy(), R.trilu(x, -2, False), "Trilu")
        same_bits(ops.Trilu().run(ctx, [dev(ctx, x)])[0].numpy(), R.trilu(x, 0, True), "Trilu, default k")
        same_bits(ops.Tile().run(ctx, [dev(ctx, x), np.array([2, 1, 3], I)])[0].numpy(), R.tile(x, [2, 1, 3]), "Tile")
    from rten_amd.tensor import DeviceTensor
    assert ops.Tile().run(ctx, [DeviceTensor.from_numpy(ctx, np.array(5, I)), np.zeros(0, I)])[0].numpy().tolist() == 5  # a scalar with no repeats


# ================================================================================================ graphs
from tests.test_gpu_sample import CLI_MODES, SESSION_TIMEOUT_S, model_run, run_cli_graph  # noqa: E402  (node by node, fused, unfused, captured and replayed)


def close_enough(got, want, what):
    """Exported graphs against torch's CPU forward: rtol = atol = 1e-4, the bound tests/test_shape_arithmetic.py and tests/test_graph_executor.py use."""
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4, err_msg=what)


def through_one_graph(ctx, tmp_path, data, bindings, compare):
    """`bindings` = [(feeds, {output: expected})] at two shapes and back at the first.  ONE loaded Graph in one process of tests/cpp/graph_session.cpp: an eager
    run at every binding (the two sizes in both orders), a capture at the first, a replay, the last binding's values written into the captured feeds and replayed,
    an eager run at the second shape again.  Then the executor behind the C ABI (fused, captured by prepare) and a clone of it on a second context."""
    from safetensors.numpy import save_file
    from rten_amd import lib as L
    from tests import graph_sessions as gs
    from tests.test_gpu_graph_fuzz import read_safetensors
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
        got = dict(read_safetensors(path))
        for name, want in bindings[binding][1].items():
            compare(got[name].reshape(want.shape), want, f"one graph, {verb} at binding {binding}, output {name}")
    m = L.Model(ctx, data)
    other = L.Context(0)
    try:
        want = bindings[0][1][m.outputs[0]]  # (model_run reads the first output)
        compare(model_run(ctx, m, bindings[0][0]).reshape(want.shape), want, "the C-ABI model")
        lane = m.clone(other)
        try:
            want = bindings[last][1][m.outputs[0]]
            compare(model_run(other, lane, bindings[last][0]).reshape(want.shape), want, "its clone on a second context")
        finally:
            lane.close()
    finally:
        m.close()
        other.close()


def index_graph_feeds(rng, batch, rows=4, cols=5, picks=3):
    x = (rng.standard_normal((batch, rows, cols)) * 10 ** rng.uniform(-2, 2, (batch, rows, cols))).astype(F)
    x[0, 0, 0] = -0.0
    return {"x": x, "m": rng.integers(-5, 6, (batch, rows, cols)).astype(I), "idx": rng.integers(-rows, rows, (batch, picks, cols)).astype(I)}


def index_graph_rules(f):
    x, m, idx = f["x"], f["m"], f["idx"]
    return {"cum_excl_rev": R.cum_sum(x, -1, True, True), "cum_mid_rev": R.cum_sum(x, 1, False, True), "cum_int_excl": R.cum_sum(m, 2, True, False),
            "cum_rows": R.cum_sum(x, 0), "gather_mid": R.gather_elements(x, idx, 1), "gather_last": R.gather_elements(x, idx, -1),
            "tril_km1": R.trilu(x, -1, False), "triu_k1": R.trilu(x, 1, True), "tiled": R.tile(x, [1, 2, 3])}


def test_writer_graph_with_every_attribute(ctx, tmp_path):
    from rten_amd import onnx_writer as ow
    data = ow.index_ops_graph()
    rng = np.random.default_rng(71)
    bindings = []
    for batch in (2, 5, 2):
        feeds = index_graph_feeds(rng, batch)
        bindings.append((feeds, index_graph_rules(feeds)))
    feeds, want = bindings[1]
    for extra in CLI_MODES:
        got, log = run_cli_graph(tmp_path, data, feeds, ow.INDEX_OPS_OUTPUTS, {"batch": 5}, extra)
        for name in ow.INDEX_OPS_OUTPUTS:
            same_bits(got[name].view(want[name].dtype).reshape(want[name].shape), want[name], f"index_ops {extra} {name}")
        if extra == ("-t",):
            for kind in ("CumSum", "GatherElements", "Trilu", "Tile"):
                assert kind in log, log[-2500:]
    through_one_graph(ctx, tmp_path, data, bindings, same_bits)


def roberta_feeds(rng, batch, seq, vocab=100, pad=1):
    """input_ids with pad tokens inside and at the end of rows: cumsum(mask) * mask + pad matters.  attention_mask masks the pads at the end."""
    ids = rng.integers(3, vocab, (batch, seq)).astype(I)
    ids[0, 2] = pad
    ids[-1, seq - 2:] = pad
    ids[-1, 1] = pad
    mask = np.ones((batch, seq), I)
    mask[-1, seq - 2:] = 0
    return {"input_ids": ids, "attention_mask": mask}


@pytest.mark.parametrize("dynamic", [False, True])
def test_roberta_export(ctx, tmp_path, dynamic):
    """transformers' RobertaModel through torch's exporter: one CumSum (position ids, int32 device data, the row form) and one GatherElements (the buffered
    token_type_ids: a host-valued data operand with device indices).  last_hidden_state against torch's CPU forward, in every run mode."""
    import torch
    import torch_export as te
    module = te.roberta_module()
    data = te.roberta_onnx(module, 2, 7, dynamic)
    rng = np.random.default_rng(81)

    def forward(f):
        with torch.no_grad():
            return module(torch.from_numpy(f["input_ids"].astype(np.int64)), torch.from_numpy(f["attention_mask"].astype(np.int64))).last_hidden_state.numpy()
    sizes = ((2, 7), (3, 12), (2, 7)) if dynamic else ((2, 7), (2, 7), (2, 7))
    bindings = []
    for batch, seq in sizes:
        feeds = roberta_feeds(rng, batch, seq)
        bindings.append((feeds, {"last_hidden_state": forward(feeds)}))
    for k in (0, 1) if dynamic else (0,):
        feeds, want = bindings[k]
        b, s = feeds["input_ids"].shape
        results = {}
        for extra in CLI_MODES:
            got, log = run_cli_graph(tmp_path, data, feeds, ["last_hidden_state"], {"batch": b, "seq": s} if dynamic else {}, extra)
            results[extra] = got["last_hidden_state"].reshape(want["last_hidden_state"].shape)
            close_enough(results[extra], want["last_hidden_state"], f"roberta {extra} at {b} x {s}")
            if extra == ("-t",):
                assert "CumSum" in log and "GatherElements" in log, log[-2500:]
        close_enough(results[()], results[("--no-fuse",)], "roberta fused against unfused")
        same_bits(results[("--graph", "-n", "2")], results[()], "roberta captured against eager")
    through_one_graph(ctx, tmp_path, data, bindings, close_enough)


@pytest.mark.parametrize("dynamic", [False, True])
def test_causal_decoder_export(ctx, tmp_path, dynamic):
    """The plain torch.nn decoder block: CumSum (position ids), Trilu (the causal mask: a constant operand statically, run-time shape arithmetic with dynamic
    axes -- host-evaluated either way), GatherElements (each row's last token) and Tile (.repeat).  y against torch's CPU forward, in every run mode."""
    import torch
    import torch_export as te
    module = te.causal_decoder_module()
    data = te.causal_decoder_onnx(module, 2, 6, dynamic)
    rng = np.random.default_rng(91)

    def feeds_for(batch, seq):
        ids = rng.integers(2, 50, (batch, seq)).astype(I)
        ids[0, 1] = te.CAUSAL_DECODER_PAD
        ids[-1, seq - 2:] = te.CAUSAL_DECODER_PAD
        return {"ids": ids}

    def forward(f):
        with torch.no_grad():
            return module(torch.from_numpy(f["ids"].astype(np.int64))).numpy()
    sizes = ((2, 6), (3, 9), (2, 6)) if dynamic else ((2, 6), (2, 6), (2, 6))
    bindings = []
    for batch, seq in sizes:
        feeds = feeds_for(batch, seq)
        bindings.append((feeds, {"y": forward(feeds)}))
    for k in (0, 1) if dynamic else (0,):
        feeds, want = bindings[k]
        b, s = feeds["ids"].shape
        results = {}
        for extra in CLI_MODES:
            got, log = run_cli_graph(tmp_path, data, feeds, ["y"], {"batch": b, "seq": s} if dynamic else {}, extra)
            results[extra] = got["y"].reshape(want["y"].shape)
            close_enough(results[extra], want["y"], f"causal decoder {extra} at {b} x {s}")
            if extra == ("-t",):
                assert "CumSum" in log and "GatherElements" in log, log[-2500:]
        close_enough(results[()], results[("--no-fuse",)], "causal decoder fused against unfused")
        same_bits(results[("--graph", "-n", "2")], results[()], "causal decoder captured against eager")
        assert np.isfinite(results[()]).all()  # the -inf of the mask stays inside the softmax
    through_one_graph(ctx, tmp_path, data, bindings, close_enough)


def test_batch_coupling_refuses_sub_batch_chains(ctx):
    """Sub-batch chains split dim 0.  CumSum / GatherElements along axis 0, a Tile that repeats dim 0 and a Trilu of a rank-2 operand couple the rows: a constant CumSum
    axis 0 and GatherElements' attribute are refused at load, a negative axis, the repeats and Trilu's rank when the probe run of prepare() sees them.  The same
    operators on inner axes are not coupled."""
    from rten_amd import lib as L
    from rten_amd import onnx_writer as ow
    i64c = lambda name, v: ow.tensor(name, np.asarray(v, np.int64))

    def model(kind, shape, operand=None, **attrs):
        ins = [ow.value_info("x", ow.FLOAT, shape)]
        second = []
        if kind == "GatherElements":
            ins.append(ow.value_info("idx", ow.INT32, shape))
            second = ["idx"]
        elif operand is not None:
            second = ["c"]
        nodes = [ow.node("Relu", ["x"], ["r"], name="relu"), ow.node(kind, ["r"] + second, ["y"], name="node", **attrs)]
        return ow.model(nodes, ins, [ow.value_info("y", ow.FLOAT, ["a", "b", "c"][:len(shape)])], [i64c("c", operand)] if operand is not None and kind != "GatherElements" else [], opset=14)

    def prepare(data, shape):
        m = L.Model(ctx, data, None, 2)
        try:
            for name in m.inputs:
                m.bind_input(name, shape)
            m.prepare()
        finally:
            m.close()

    free, coupled = [], []
    free.append((model("CumSum", ["batch", 3, 5], 1), (4, 3, 5)))
    free.append((model("CumSum", ["batch", 3, 5], -1), (4, 3, 5)))
    free.append((model("GatherElements", ["batch", 3, 5], axis=2), (4, 3, 5)))
    free.append((model("Trilu", ["batch", 3, 5], 1), (4, 3, 5)))
    free.append((model("Tile", ["batch", 3, 5], [1, 2, 3]), (4, 3, 5)))
    coupled.append((model("CumSum", ["batch", 3, 5], 0), (4, 3, 5), "CumSum"))
    coupled.append((model("CumSum", ["batch", 3, 5], -3), (4, 3, 5), 'CumSum "node" (sums along dim 0)'))
    coupled.append((model("GatherElements", ["batch", 3, 5], axis=0), (4, 3, 5), "GatherElements"))
    coupled.append((model("GatherElements", ["batch", 3, 5], axis=-3), (4, 3, 5), "GatherElements"))
    coupled.append((model("Trilu", ["batch", 5]), (4, 5), 'Trilu "node" (dim 0 is the matrix row)'))
    coupled.append((model("Tile", ["batch", 3, 5], [2, 1, 1]), (4, 3, 5), 'Tile "node" (repeats dim 0)'))
    for data, shape in free:
        prepare(data, shape)
    for data, shape, words in coupled:
        with pytest.raises(L.HipError) as e:
            prepare(data, shape)
        assert words in str(e.value) and '"node"' in str(e.value) and "couples the rows" in str(e.value), str(e.value)
