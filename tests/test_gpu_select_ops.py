"""ReduceMax / ReduceMin / ArgMax / ArgMin / TopK on the device, bit-exact against the numpy restatement of the rules (tests/select_rules.py): values as
bit patterns after mapping every NaN to one NaN (and, for ReduceMax / ReduceMin only, -0 to +0), indices exactly.  The operators are driven through
rten_amd.ops on strided views, i.e. through the three C-ABI entry points of rten_amd/csrc/select.hip."""
import os
import sys

import numpy as np
import pytest

from rten_amd import einsum as E
from rten_amd import onnx_writer as ow
from rten_amd import ops
from rten_amd.tensor import DeviceTensor
from tests import select_rules as R

pytestmark = pytest.mark.gpu

NAN = np.float32("nan")
ROW_LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4096, 8193, 151936]
LANE_COUNTS = [1, 3, 64, 49152]
MAX_ELEMS = 1 << 26  # 256 MB of 4-byte elements


def same(got, want, fold_zero_sign=False, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = R.canon(got, fold_zero_sign), R.canon(want, fold_zero_sign)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f"{what}: {len(bad)} of {g.size} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


def dview(ctx, base, view):
    """Uploads `base` and returns the einsum.View that addresses what the numpy view `view` of it addresses (a transposed / sliced operand)."""
    t = DeviceTensor.from_numpy(ctx, base)
    off = (view.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // 4 if view.size else 0
    assert all(s % 4 == 0 and s >= 0 for s in view.strides)
    sub = DeviceTensor(ctx, (max(base.size - off, 0),), base.dtype, ptr=t.ptr + 4 * off, keepalive=t)
    return E.View(sub, list(view.shape), [s // 4 for s in view.strides])


def rule_data(shape, dtype, seed, nans="some"):
    """Heavy ties (4 distinct numbers), +-0, +-inf, denormals / int32 extremes; NaNs: "none", "some" (~1 %)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape, dtype=np.int64))
    if np.dtype(dtype) == np.int32:
        x = rng.choice(np.array([-7, 0, 3, 3000], np.int32), n)
        s = rng.random(n)
        x[s < 0.01] = np.iinfo(np.int32).min
        x[(s >= 0.01) & (s < 0.02)] = np.iinfo(np.int32).max
        return x.reshape(shape)
    x = rng.choice(np.array([-1.5, 0.0, -0.0, 2.0], np.float32), n)
    s = rng.random(n)
    for i, v in enumerate([np.inf, -np.inf, 1e-40, -1e-40, 3.0e38, -0.0]):
        x[(s >= 0.01 * i) & (s < 0.01 * (i + 1))] = np.float32(v)
    if nans == "some":
        x[s > 0.99] = NAN
    return x.reshape(shape)


def lane_matrix(lanes, length, dtype, seed):
    """[lanes, length]: distinct-ish values with ties; lane r % 8: 1 = a NaN first, 2 = in the middle, 3 = last, 4 = all equal, 5 = all zeros of both signs, else no NaN
    (at most one NaN per lane, so TopK indices are comparable)."""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.int32:
        x = rng.integers(-50, 50, size=(lanes, length)).astype(np.int32)
        x[rng.random((lanes, length)) < 0.001] = np.iinfo(np.int32).min
        x[rng.random((lanes, length)) < 0.001] = np.iinfo(np.int32).max
        x[4::8] = 11
        return x
    x = (rng.integers(-2000, 2000, size=(lanes, length)) / np.float32(8)).astype(np.float32)
    x[rng.random((lanes, length)) < 0.001] = np.float32(np.inf)
    x[rng.random((lanes, length)) < 0.001] = np.float32(-np.inf)
    x[rng.random((lanes, length)) < 0.001] = np.float32(1e-41)
    x[1::8, 0] = NAN
    x[2::8, length // 2] = NAN
    x[3::8, length - 1] = NAN
    x[4::8] = np.float32(-3.25)
    x[5::8] = np.where(rng.random((len(x[5::8]), length)) < 0.5, np.float32(0.0), np.float32(-0.0))
    return x


def check_reduce_and_arg(ctx, base, view, axes_sets, what):
    v = dview(ctx, base, view)
    for axes in axes_sets:
        for keep in (True, False):
            for cls, op in ((ops.ReduceMax, "max"), (ops.ReduceMin, "min")):
                got = cls(axes=axes, keep_dims=keep).run(ctx, [v])[0].numpy()
                same(got, R.reduce_minmax(view, axes, keep, op), True, f"{what} {cls.__name__} axes={axes} keep={keep}")
            if axes is not None and len(axes) == 1:
                for cls, op in ((ops.ArgMax, "max"), (ops.ArgMin, "min")):
                    got = cls(axis=axes[0], keep_dims=keep).run(ctx, [v])[0].numpy()
                    same(got, R.arg_minmax(view, axes[0], keep, op), False, f"{what} {cls.__name__} axis={axes[0]} keep={keep}")


@pytest.mark.parametrize("dtype", [np.float32, np.int32])
def test_ranks_axes_keepdims(ctx, dtype):
    shapes = [(37,), (9, 21), (5, 6, 7), (3, 4, 5, 6), (2, 3, 4, 3, 5)]
    multi = {2: [[0, 1]], 3: [[0, 2], [1, 2], [-1, 0, 1]], 4: [[1, 3], [0, 1], [2, 3], [0, 2, 3]], 5: [[0, 4], [1, 2, 3], [0, 2, 4], [3, 4]]}
    for shape in shapes:
        nd = len(shape)
        x = rule_data(shape, dtype, seed=nd)
        axes_sets = [None] + [[a] for a in range(nd)] + [[-1]] + multi.get(nd, [])
        check_reduce_and_arg(ctx, x, x, axes_sets, f"contiguous {shape}")
        if nd >= 2:
            perm = tuple(reversed(range(nd)))
            check_reduce_and_arg(ctx, x, x.transpose(perm), axes_sets, f"transposed {shape}")
            sl = tuple(slice(1, None, 2) if d == nd - 1 else slice(0, s - 1) if s > 2 else slice(None) for d, s in enumerate(shape))
            check_reduce_and_arg(ctx, x, x[sl], axes_sets, f"sliced {shape}")


def test_zero_d_and_empty(ctx):
    for dtype in (np.float32, np.int32):
        s = np.array(5, dtype)
        same(ops.ReduceMax().run(ctx, [DeviceTensor.from_numpy(ctx, s)])[0].numpy(), s)
        e = np.zeros((4, 0, 3), dtype)
        for cls, op in ((ops.ReduceMax, "max"), (ops.ReduceMin, "min")):
            same(cls(axes=[1]).run(ctx, [DeviceTensor.from_numpy(ctx, e)])[0].numpy(), R.reduce_minmax(e, [1], True, op))
            same(cls(axes=[0], keep_dims=False).run(ctx, [DeviceTensor.from_numpy(ctx, e)])[0].numpy(), R.reduce_minmax(e, [0], False, op))
        with pytest.raises(ops.OpError) as err:
            ops.ArgMax(axis=1).run(ctx, [DeviceTensor.from_numpy(ctx, e)])
        assert err.value == ops.InvalidValue("Cannot select index from empty sequence")
    same(ops.ArgMax(axis=0, keep_dims=False).run(ctx, [DeviceTensor.from_numpy(ctx, np.array([1, 3, 3], np.float32))])[0].numpy(), np.array(2, np.int32))
    same(ops.ArgMin(axis=0, keep_dims=False).run(ctx, [DeviceTensor.from_numpy(ctx, np.array([2, 1, 1], np.float32))])[0].numpy(), np.array(2, np.int32))
    same(ops.ArgMax(axis=0, keep_dims=False).run(ctx, [DeviceTensor.from_numpy(ctx, np.array([NAN, 5, NAN], np.float32))])[0].numpy(), np.array(0, np.int32))
    same(ops.ArgMin(axis=0, keep_dims=False).run(ctx, [DeviceTensor.from_numpy(ctx, np.array([NAN, 5, NAN], np.float32))])[0].numpy(), np.array(0, np.int32))
    same(ops.ArgMax(axis=0, keep_dims=False).run(ctx, [DeviceTensor.from_numpy(ctx, np.array([-0.0, 0.0], np.float32))])[0].numpy(), np.array(1, np.int32))
    same(ops.ArgMax(axis=0, keep_dims=False).run(ctx, [DeviceTensor.from_numpy(ctx, np.array([0.0, -0.0], np.float32))])[0].numpy(), np.array(1, np.int32))


def sampled_pairs():
    """Every row length with two of the lane counts (rotating, plus the largest that keeps the input under 256 MB)."""
    pairs = []
    for i, length in enumerate(ROW_LENGTHS):
        fits = [n for n in LANE_COUNTS if n * length <= MAX_ELEMS]
        pairs.append((length, fits[i % len(fits)]))
        if (length, fits[-1]) not in pairs:
            pairs.append((length, fits[-1]))
    return pairs + [(151936, 1), (4096, 1)]  # a lone long lane: the launch-bound case


@pytest.mark.parametrize("length,lanes", sampled_pairs())
def test_row_lengths_and_lane_counts(ctx, length, lanes):
    dtype = np.int32 if (length + lanes) % 5 == 0 else np.float32  # int32 on a fifth of the pairs; the others float32
    x = lane_matrix(lanes, length, dtype, seed=length * 7 + lanes)
    # the reduced axis contiguous ([lanes, length], axis 1) and strided with a contiguous kept axis (the transposed buffer, axis 0)
    xt = np.ascontiguousarray(x.T)
    for base, axis, name in ((x, 1, "last axis"), (xt, 0, "strided axis")):
        t = DeviceTensor.from_numpy(ctx, base)
        for cls, op in ((ops.ReduceMax, "max"), (ops.ReduceMin, "min")):
            got = cls(axes=[axis], keep_dims=False).run(ctx, [t])[0].numpy()
            same(got, R.reduce_minmax(base, [axis], False, op), True, f"{name} {cls.__name__} {lanes} x {length} {np.dtype(dtype).name}")
        for cls, op in ((ops.ArgMax, "max"), (ops.ArgMin, "min")):
            got = cls(axis=axis, keep_dims=False).run(ctx, [t])[0].numpy()
            same(got, R.arg_minmax(base, axis, False, op), False, f"{name} {cls.__name__} {lanes} x {length} {np.dtype(dtype).name}")
        t.free()


@pytest.mark.parametrize("dtype", [np.float32, np.int32])
def test_whole_tensor_reduction(ctx, dtype):
    shape = (4099, 4101)  # > 2^24 elements, rows not a multiple of 4 elements
    rng = np.random.default_rng(5)
    x = rng.integers(-(1 << 20), 1 << 20, size=shape).astype(dtype)
    x[3011, 1234], x[17, 4100] = 1 << 21, -(1 << 21)
    t = DeviceTensor.from_numpy(ctx, x)
    for keep in (True, False):
        same(ops.ReduceMax(keep_dims=keep).run(ctx, [t])[0].numpy(), R.reduce_minmax(x, None, keep, "max"))
        same(ops.ReduceMin(keep_dims=keep).run(ctx, [t])[0].numpy(), R.reduce_minmax(x, None, keep, "min"))
    flat = t.reshape(x.size)
    same(ops.ArgMax(axis=0, keep_dims=False).run(ctx, [flat])[0].numpy(), R.arg_minmax(x.reshape(-1), 0, False, "max"))
    same(ops.ArgMin(axis=0, keep_dims=False).run(ctx, [flat])[0].numpy(), R.arg_minmax(x.reshape(-1), 0, False, "min"))
    if dtype == np.float32:  # one NaN in the last chunk: it wins everything
        x[4098, 4000] = NAN
        t.upload(x)
        assert np.isnan(ops.ReduceMax(keep_dims=False).run(ctx, [t])[0].numpy()) and np.isnan(ops.ReduceMin(keep_dims=False).run(ctx, [t])[0].numpy())
        same(ops.ArgMin(axis=0, keep_dims=False).run(ctx, [flat])[0].numpy(), np.array(4098 * 4101 + 4000, np.int32))
    # ties across chunks: the last of the equal extremes
    x[...] = 7
    t.upload(x)
    same(ops.ArgMax(axis=0, keep_dims=False).run(ctx, [flat])[0].numpy(), np.array(x.size - 1, np.int32))


def check_topk(ctx, v, view, k, axis, largest, sorted_, what, indices=True):
    got_v, got_i = [o.numpy() for o in ops.TopK(axis=axis, largest=largest, sorted=sorted_).run(ctx, [v, np.array([k], np.int32)])]
    want_v, want_i = R.topk(view, k, axis, largest)
    if not sorted_:  # any order of the same (value, index) pairs: compare as sets per lane
        ax = axis if axis >= 0 else axis + view.ndim
        order = np.argsort(got_i, axis=ax, kind="stable")
        got_v, got_i = np.take_along_axis(got_v, order, ax), np.take_along_axis(got_i, order, ax)
        order = np.argsort(want_i, axis=ax, kind="stable")
        want_v, want_i = np.take_along_axis(want_v, order, ax), np.take_along_axis(want_i, order, ax)
    same(got_v, want_v, False, f"{what} values k={k} axis={axis} largest={largest} sorted={sorted_}")
    if indices:
        same(got_i, want_i, False, f"{what} indices k={k} axis={axis} largest={largest} sorted={sorted_}")
    else:
        assert got_i.shape == want_i.shape and got_i.dtype == np.int32
        assert np.array_equal(R.canon(np.take_along_axis(view, got_i.astype(np.int64), axis)), R.canon(got_v)), f"{what}: indices do not address the values"


@pytest.mark.parametrize("length,lanes", [(1, 3), (5, 64), (17, 3), (300, 64), (1000, 32), (4096, 3), (8192, 2), (8193, 3), (20000, 8), (151936, 3)])
def test_topk_last_axis(ctx, length, lanes):
    for dtype in ((np.float32, np.int32) if length in (5, 1000, 8193) else (np.float32,)):
        x = lane_matrix(lanes, length, dtype, seed=length + 1)
        t = DeviceTensor.from_numpy(ctx, x)
        for k in sorted({k for k in (0, 1, 5, 300, 4096, length) if k <= length and k <= 4096}):
            for largest in (True, False):
                check_topk(ctx, t, x, k, -1, largest, True, f"{lanes} x {length} {np.dtype(dtype).name}")
            check_topk(ctx, t, x, k, 1, k % 2 == 0, False, f"{lanes} x {length} {np.dtype(dtype).name}")


def test_topk_other_axes_and_views(ctx):
    x = lane_matrix(6 * 5, 700, np.float32, seed=3).reshape(6, 5, 700)
    xt = np.ascontiguousarray(x.transpose(2, 0, 1))  # [700, 6, 5]: the selected axis is the outermost, lanes contiguous
    t = DeviceTensor.from_numpy(ctx, xt)
    for k in (1, 5, 300, 700):
        for largest in (True, False):
            check_topk(ctx, t, xt, k, 0, largest, True, "axis 0 of [700, 6, 5]")
    xm = np.ascontiguousarray(x.transpose(0, 2, 1))  # [6, 700, 5]: a middle axis
    t = DeviceTensor.from_numpy(ctx, xm)
    check_topk(ctx, t, xm, 8, 1, True, True, "axis 1 of [6, 700, 5]")
    check_topk(ctx, t, xm, 8, -2, False, False, "axis -2 of [6, 700, 5]")
    # a transposed and sliced view of the same buffer
    view = x.transpose(1, 0, 2)[:, 1:5, 3:699:2]
    check_topk(ctx, dview(ctx, x, view), view, 5, 2, True, True, "sliced view")
    check_topk(ctx, dview(ctx, x, view), view, 3, 1, False, True, "sliced view")
    # the matrix of the reference's own test: axis 0
    m = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.float32)
    v, i = [o.numpy() for o in ops.TopK(axis=0).run(ctx, [DeviceTensor.from_numpy(ctx, m), np.array(2, np.int32)])]
    same(v, np.array([[6, 7, 8], [3, 4, 5]], np.float32))
    same(i, np.array([[2, 2, 2], [1, 1, 1]], np.int32))


def test_topk_rule_data_and_several_nans(ctx):
    # heavy ties, +-0, +-inf, denormals, no NaN: indices are fully determined by "smaller index first"
    for length in (64, 1000, 9000):
        x = rule_data((7, length), np.float32, seed=length, nans="none")
        t = DeviceTensor.from_numpy(ctx, x)
        for k in (1, 5, min(300, length), min(length, 4096)):
            for largest in (True, False):
                check_topk(ctx, t, x, k, -1, largest, True, f"ties {length}")
        xi = rule_data((7, length), np.int32, seed=length)
        check_topk(ctx, DeviceTensor.from_numpy(ctx, xi), xi, min(length, 300), -1, True, True, f"int ties {length}")
        check_topk(ctx, DeviceTensor.from_numpy(ctx, xi), xi, min(length, 300), -1, False, True, f"int ties {length}")
    # several NaNs per lane: values only (the reference's comparator is inconsistent there; the device orders NaNs by ascending index)
    for length in (100, 5000, 40000):
        x = rule_data((5, length), np.float32, seed=length + 1, nans="some")
        t = DeviceTensor.from_numpy(ctx, x)
        for k in (5, 100, min(length, 4096)):
            for largest in (True, False):
                check_topk(ctx, t, x, k, -1, largest, True, f"several NaNs {length}", indices=False)


def test_topk_errors_and_large_k(ctx):
    x = lane_matrix(2, 10000, np.float32, seed=9)
    t = DeviceTensor.from_numpy(ctx, x)
    K = lambda k: np.array([k], np.int32)
    for bad, msg in ((10001, "k > dimension size"), (-1, "k must be positive")):
        with pytest.raises(ops.OpError) as err:
            ops.TopK().run(ctx, [t, K(bad)])
        assert err.value == ops.InvalidValue(msg)
    # k > 4096 on a long lane: the documented refusal, or the right answer -- never a wrong one
    try:
        got = [o.numpy() for o in ops.TopK().run(ctx, [t, K(5000)])]
    except ops.OpError as e:
        assert e.kind == "UnsupportedValue" and "k > 4096" in e.msg, e
    else:
        want = R.topk(x, 5000, -1, True)
        same(got[0], want[0])
        same(got[1], want[1])
    v, i = ops.TopK().run(ctx, [t, K(0)])
    assert v.shape == i.shape == (2, 0)


# ---------------------------------------------------------------------------------------------------- graphs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("-t",), ("--no-fuse",), ("--graph", "-n", "2"))  # fused, unfused, captured and replayed


def run_graph(tmp_path, model_bytes, inputs, outs, *extra):
    """Runs the executor CLI; `outs` = {name: (dtype, shape)}: the dumped raw bytes of every output, typed and shaped."""
    from tests.test_graph_executor import run_cli
    p = tmp_path / "m.onnx"
    p.write_bytes(model_bytes)
    args = []
    for name, arr in inputs.items():
        f = tmp_path / f"{name}.bin"
        arr.tofile(f)
        args += ["--input", f"{name}={f}"]
    for o in outs:
        args += ["--dump", f"{o}={tmp_path / (o + '.bin')}"]
    r = run_cli("-s", f"batch={next(iter(inputs.values())).shape[0]}", *args, *extra, str(p))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return {o: np.fromfile(tmp_path / (o + ".bin"), dt).reshape(shape) for o, (dt, shape) in outs.items()}, r.stdout


def torch_export():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export as te
    return te


def no_ties_no_nan(x, axis):
    """The precondition under which torch and the reference agree on indices: no NaN, and no two equal values along `axis`."""
    s = np.sort(x, axis=axis)
    return not np.isnan(x).any() and bool((np.diff(s, axis=axis) != 0).all())


def test_classifier_head_softmax_topk(tmp_path):
    import torch
    te = torch_export()
    data = te.classifier_topk_onnx()
    x = np.random.default_rng(11).standard_normal((3, 3, 32, 32)).astype(np.float32)
    outs = {"probs": (np.float32, (3, 10)), "values": (np.float32, (3, 5)), "indices": (np.int32, (3, 5))}
    first = None
    for mode in MODES:
        got, log = run_graph(tmp_path, data, {"x": x}, outs, *mode)
        wv, wi = R.topk(got["probs"], 5, -1, True)
        same(got["values"], wv, False, f"values {mode}")
        same(got["indices"], wi, False, f"indices {mode}")
        if mode == ("-t",):
            assert any(line.split() and line.split()[0] == "TopK" for line in log.splitlines()), log[-3000:]
        first = first or got
        for o in outs:
            same(got[o], first[o], False, f"{o} {mode} vs fused")
    assert no_ties_no_nan(first["probs"], 1)
    assert np.array_equal(torch.topk(torch.from_numpy(first["probs"]), 5).indices.numpy(), first["indices"])


def test_segmentation_head_interpolate_argmax(tmp_path):
    import torch
    te = torch_export()
    data = te.segment_argmax_onnx()
    x = np.random.default_rng(12).standard_normal((3, 3, 32, 32)).astype(np.float32)
    outs = {"logits": (np.float32, (3, 21, 32, 32)), "labels": (np.int32, (3, 32, 32))}
    first = None
    for mode in MODES:
        got, log = run_graph(tmp_path, data, {"x": x}, outs, *mode)
        same(got["labels"], R.arg_minmax(got["logits"], 1, False, "max"), False, f"labels {mode}")
        if mode == ("-t",):
            assert any(line.split() and line.split()[0] == "ArgMax" for line in log.splitlines()), log[-3000:]
        first = first or got
        for o in outs:
            same(got[o], first[o], False, f"{o} {mode} vs fused")
    assert not np.isnan(first["logits"]).any() and ((first["logits"] == first["logits"].max(1, keepdims=True)).sum(1) == 1).all()  # one maximum per pixel
    assert np.array_equal(torch.from_numpy(first["logits"]).argmax(1).numpy(), first["labels"])


def test_yolo_head_with_in_graph_filter(tmp_path):
    import torch
    te = torch_export()
    keep, classes, anchors = 20, 4, 256
    data = te.yolo_filter_onnx()
    x = np.random.default_rng(13).standard_normal((2, 3, 64, 64)).astype(np.float32)
    outs = {"y": (np.float32, (2, 4 + classes, anchors)), "conf": (np.float32, (2, anchors)), "top": (np.float32, (2, keep)), "idx": (np.int32, (2, keep)),
            "boxes": (np.float32, (2, 4, keep)), "classes": (np.int32, (2, keep))}
    first = None
    for mode in MODES:
        got, log = run_graph(tmp_path, data, {"x": x}, outs, *mode)
        scores = got["y"][:, 4:, :]
        conf, cls = R.reduce_minmax(scores, [1], False, "max"), R.arg_minmax(scores, 1, False, "max")
        top, idx = R.topk(conf, keep, 1, True)
        same(got["conf"], conf, True, f"conf {mode}")
        same(got["top"], top, False, f"top {mode}")
        same(got["idx"], idx, False, f"idx {mode}")
        same(got["boxes"], np.take_along_axis(got["y"][:, :4, :], idx[:, None, :].astype(np.int64), 2), False, f"boxes {mode}")
        same(got["classes"], np.take_along_axis(cls, idx.astype(np.int64), 1), False, f"classes {mode}")
        if mode == ("-t",):
            kinds = {line.split()[0] for line in log.splitlines() if line.split()}
            assert {"ReduceMax", "ArgMax", "TopK"} <= kinds, log[-3000:]
        first = first or got
        for o in outs:
            same(got[o], first[o], False, f"{o} {mode} vs fused")
    assert no_ties_no_nan(first["conf"], 1) and no_ties_no_nan(first["y"][:, 4:, :], 1)
    ty = torch.from_numpy(first["y"])
    tconf, tcls = ty[:, 4:, :].max(1)
    ttop, tidx = tconf.topk(keep, dim=1)
    assert np.array_equal(tidx.numpy(), first["idx"]) and np.array_equal(torch.gather(tcls, 1, tidx).numpy(), first["classes"])


def test_graphs_that_must_not_load(tmp_path):
    from tests.test_graph_executor import run_cli
    x = np.arange(12, dtype=np.float32).reshape(2, 6)
    xf = tmp_path / "x.bin"
    x.tofile(xf)
    # K as a graph input: device data at run time
    m = ow.model([ow.node("TopK", ["x", "k"], ["v", "i"], name="topk_runtime_k")],
                 [ow.value_info("x", ow.FLOAT, [2, 6]), ow.value_info("k", ow.INT64, [1])],
                 [ow.value_info("v", ow.FLOAT, []), ow.value_info("i", ow.INT64, [])], [], opset=13)
    p = tmp_path / "k.onnx"
    p.write_bytes(m)
    kf = tmp_path / "k.bin"
    np.array([2], np.int32).tofile(kf)
    r = run_cli("--input", f"x={xf}", "--input", f"k={kf}", str(p))
    assert r.returncode != 0 and "topk_runtime_k" in r.stderr and "K must be a constant" in r.stderr, r.stderr[-1500:]
    for kind in ("ArgMax", "ArgMin"):
        m = ow.model([ow.node(kind, ["x"], ["i"], name="arg_last_index", axis=1, select_last_index=1)], [ow.value_info("x", ow.FLOAT, [2, 6])],
                     [ow.value_info("i", ow.INT64, [])], [], opset=13)
        p = tmp_path / "a.onnx"
        p.write_bytes(m)
        r = run_cli("--input", f"x={xf}", str(p))
        assert r.returncode != 0 and "arg_last_index" in r.stderr and "select_last_index" in r.stderr, r.stderr[-1500:]


def test_graph_forms_of_the_five_operators(tmp_path):
    """Hand-written nodes: axes as attribute (opset 13) and as input (opset 18), keepdims, K from an initializer, int32 data through Cast, min forms."""
    x = lane_matrix(6, 40, np.float32, seed=21).reshape(2, 3, 40)
    x[0, 1, 7] = x[0, 1, 9] = np.float32(500.0)  # a tie for the maximum: the later index
    nodes = [ow.node("ReduceMax", ["x"], ["rmax"], name="rmax", axes=[1], keepdims=0),
             ow.node("ReduceMin", ["x"], ["rmin"], name="rmin", axes=[-1, 0], keepdims=1),
             ow.node("ArgMax", ["x"], ["amax"], name="amax", axis=2, keepdims=0),
             ow.node("ArgMin", ["x"], ["amin"], name="amin", axis=-2),
             ow.node("TopK", ["x", "k"], ["tv", "ti"], name="topk", axis=2, largest=0),
             ow.node("Cast", ["x"], ["xi"], name="cast", to=ow.INT32),
             ow.node("TopK", ["xi", "k"], ["iv", "ii"], name="topk_int", axis=1),
             ow.node("ReduceMax", ["xi"], ["imax"], name="imax", keepdims=0)]
    outs = {"rmax": (np.float32, (2, 40)), "rmin": (np.float32, (1, 3, 1)), "amax": (np.int32, (2, 3)), "amin": (np.int32, (2, 1, 40)),
            "tv": (np.float32, (2, 3, 3)), "ti": (np.int32, (2, 3, 3)), "iv": (np.int32, (2, 3, 40)), "ii": (np.int32, (2, 3, 40)), "imax": (np.int32, ())}
    m = ow.model(nodes, [ow.value_info("x", ow.FLOAT, [2, 3, 40])], [ow.value_info(o, {"amax": ow.INT64, "amin": ow.INT64, "ti": ow.INT64, "ii": ow.INT64, "iv": ow.INT32, "imax": ow.INT32}.get(o, ow.FLOAT), []) for o in outs],
                 [ow.tensor("k", np.array([3], np.int64))], opset=13)
    xs = x.copy()
    xs[np.isnan(xs) | np.isinf(xs)] = 1.0  # (the Cast to int32 of NaN / inf is its own subject)
    xi = xs.astype(np.int32)
    want = {"rmax": R.reduce_minmax(xs, [1], False, "max"), "rmin": R.reduce_minmax(xs, [-1, 0], True, "min"), "amax": R.arg_minmax(xs, 2, False, "max"),
            "amin": R.arg_minmax(xs, -2, True, "min"), "imax": R.reduce_minmax(xi, None, False, "max")}
    want["tv"], want["ti"] = R.topk(xs, 3, 2, False)
    want["iv"], want["ii"] = R.topk(xi, 3, 1, True)
    for mode in MODES:
        got, _ = run_graph(tmp_path, m, {"x": xs}, outs, *mode)
        for o in outs:
            same(got[o], want[o], o in ("rmax", "rmin"), f"{o} {mode}")
    # opset 18: axes as the second input
    m18 = ow.model([ow.node("ReduceMax", ["x", "ax"], ["rmax"], name="rmax18", keepdims=0)], [ow.value_info("x", ow.FLOAT, [2, 3, 40])],
                   [ow.value_info("rmax", ow.FLOAT, [])], [ow.tensor("ax", np.array([1], np.int64))], opset=18)
    got, _ = run_graph(tmp_path, m18, {"x": x}, {"rmax": (np.float32, (2, 40))})
    same(got["rmax"], R.reduce_minmax(x, [1], False, "max"), True, "opset 18")
