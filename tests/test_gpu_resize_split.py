"""Resize / Upsample / Split on the device: rten_hip_resize_f32 over every mode, the host operators, and whole graphs through rten_hip_run.
Expected values are numpy restatements of src/ops/resize.rs:48-408,610-652 and src/ops/split.rs:34-136, one rounded f32 operation at a time;
comparisons are bitwise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import ref
from rten_amd import lib as L
from rten_amd import ops
from rten_amd import onnx_writer as ow
from rten_amd.tensor import DeviceTensor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
COORDS = ["half_pixel", "asymmetric", "align_corners", "pytorch_half_pixel"]
NEAREST = ["round_prefer_floor", "round_prefer_ceil", "floor", "ceil"]


def assert_bits(got, want, what=""):
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    bad = np.flatnonzero(got[~nan].view(np.int32) != want[~nan].view(np.int32))
    if bad.size:
        raise AssertionError(f"{what}: {bad.size} elements differ, first got {got[~nan][bad[0]]!r} want {want[~nan][bad[0]]!r}")


# ---------------------------------------------------------------------------------------------------- numpy restatement of resize.rs
def np_coord(d, s, coord, lin, lout):
    """input_coord (resize.rs:48-75), then f32::clamp(0, lin - 1) (NaN stays NaN)."""
    df, s = np.asarray(d, np.int64).astype(np.float32), F(s)
    with np.errstate(all="ignore"):
        if coord == "asymmetric":
            c = s * df
        elif coord == "align_corners":
            c = df * F(lin - 1) / F(lout - 1)
        elif coord == "pytorch_half_pixel" and lout <= 1:
            c = np.zeros_like(df)
        else:
            c = s * (df + F(0.5)) - F(0.5)
    hi = F(lin) - F(1)
    c = np.where(c < F(0), F(0), c)
    return np.where(c > hi, hi, c).astype(np.float32)


def np_index(c):
    """`c as usize` of a clamped coordinate: truncation, NaN -> 0."""
    return np.where(np.isnan(c), F(0), c).astype(np.int64)


def np_round(c, mode):
    """round_coord (resize.rs:121-141); f32::round rounds half away from zero (c >= 0 here)."""
    with np.errstate(invalid="ignore"):
        t = np.trunc(c)
        fr = c - t
        rnd = np.where(fr >= F(0.5), t + F(1), t)
        if mode == "ceil":
            return np.ceil(c)
        if mode == "floor":
            return c
        if mode == "round_prefer_ceil":
            return np.where(fr == F(0.5), np.ceil(c), rnd)
        return np.where(fr == F(0.5), np.floor(c), rnd)


def np_resize_planes(x, oh, ow, sy, sx, mode, coord="half_pixel", nearest="round_prefer_floor"):
    """nearest_resize / bilinear_resize (resize.rs:110-243) of [planes, ih, iw]."""
    _, ih, iw = x.shape
    cy, cx = np_coord(np.arange(oh), sy, coord, ih, oh), np_coord(np.arange(ow), sx, coord, iw, ow)
    if mode == "nearest":
        return x[:, np_index(np_round(cy, nearest))][:, :, np_index(np_round(cx, nearest))]
    y1, x1 = np_index(cy), np_index(cx)
    y2, x2 = np.minimum(y1 + 1, ih - 1), np.minimum(x1 + 1, iw - 1)
    wy, wx = (cy - y1.astype(np.float32))[None, :, None], (cx - x1.astype(np.float32))[None, None, :]
    with np.errstate(all="ignore"):
        def lerp(a, b, w):
            return (F(1) - w) * a + w * b
        top = lerp(x[:, y1][:, :, x1], x[:, y1][:, :, x2], wx)
        bottom = lerp(x[:, y2][:, :, x1], x[:, y2][:, :, x2], wx)
        return lerp(top, bottom, wy).astype(np.float32)


def np_resize(x, scales=None, sizes=None, mode="nearest", coord="half_pixel", nearest="round_prefer_floor"):
    """calc_output_size + resize_impl (resize.rs:273-408)."""
    x = np.asarray(x, np.float32)
    out, inv = [], []
    with np.errstate(all="ignore"):
        for d, n in enumerate(x.shape):
            if scales is not None:
                out.append(int(np.floor(F(n) * F(scales[d]))))
                inv.append(F(1) / F(scales[d]))
            else:
                out.append(int(sizes[d]))
                inv.append(F(n) / F(sizes[d]))
    s, o = x.shape, tuple(out)
    if o == s:
        return x.copy()
    if x.ndim == 4 and s[:2] == o[:2]:
        planes, oh, ow, sy, sx = x.reshape(s[0] * s[1], s[2], s[3]), o[2], o[3], inv[2], inv[3]
    elif x.ndim == 3 and s[:2] == o[:2]:
        planes, oh, ow, sy, sx = x.reshape(s[0] * s[1], 1, s[2]), 1, o[2], F(1), inv[2]
    elif x.ndim == 3 and s[0] == o[0]:
        planes, oh, ow, sy, sx = x, o[1], o[2], inv[1], inv[2]
    elif x.ndim == 2:
        planes, oh, ow, sy, sx = x[None], o[0], o[1], inv[0], inv[1]
    else:
        planes, oh, ow, sy, sx = x.reshape(1, 1, -1), 1, o[0], F(1), inv[0]
    if 0 in o:
        return np.zeros(o, np.float32)
    return np_resize_planes(planes, oh, ow, sy, sx, mode, coord, nearest).reshape(o)


def with_specials(x, rng):
    """NaN / inf / -0 sprinkled in: a zero lerp weight times an infinite neighbour is NaN in the reference too."""
    x = x.copy().ravel()
    idx = rng.choice(x.size, size=max(x.size // 40, 1), replace=False)
    x[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 3.4e38], np.float32), size=idx.size)
    return x


def run_kernel(ctx, x, oh, ow, sy, sx, mode, coord, nearest, y_offset=0):
    """rten_hip_resize_f32 writing `y_offset` floats into its output buffer (offset 1: no vector stores)."""
    p, ih, iw = x.shape
    xd = DeviceTensor.from_numpy(ctx, x)
    yd = DeviceTensor.from_numpy(ctx, np.full(p * oh * ow + y_offset + 4, 7.0, np.float32))  # a guard tail: nothing past the output is written
    ctx.call("rten_hip_resize_f32", ops.RESIZE_MODES[mode], ops.RESIZE_COORDS[coord], ops.RESIZE_NEAREST[nearest], p, ih, iw, oh, ow, float(sy), float(sx),
             xd.vp, C.c_void_p(yd.ptr + 4 * y_offset))
    y = yd.numpy()
    assert np.all(y[:y_offset] == 7.0) and np.all(y[y_offset + p * oh * ow:] == 7.0), "write outside the output"
    return y[y_offset:y_offset + p * oh * ow].reshape(p, oh, ow)


# (planes, in_h, in_w, out_h, out_w): 2x up, non-integer up / down, odd widths and plane counts, H = 1, an output of 1 x 1 (align_corners: 0 / 0)
GEOMS = [(3, 5, 8, 10, 16), (2, 8, 9, 3, 5), (5, 4, 6, 9, 13), (1, 1, 9, 1, 4), (3, 6, 5, 1, 1), (7, 13, 11, 26, 22), (2, 33, 65, 17, 129),
         (4, 7, 7, 7, 7), (300, 2, 3, 5, 2)]


def test_kernel_every_mode_coordinate_and_nearest_mode(ctx):
    rng = np.random.default_rng(1)
    for p, ih, iw, oh, ow in GEOMS:
        x = with_specials(rng.standard_normal(p * ih * iw).astype(np.float32), rng).reshape(p, ih, iw)
        for sy, sx in ((F(ih) / F(oh), F(iw) / F(ow)), (F(1) / F(2.5), F(1) / F(1.75))):  # sizes form, and scales unrelated to the sizes
            for coord in COORDS:
                for nearest in NEAREST:
                    want = np_resize_planes(x, oh, ow, sy, sx, "nearest", coord, nearest)
                    assert_bits(run_kernel(ctx, x, oh, ow, sy, sx, "nearest", coord, nearest), want, f"nearest {coord} {nearest} {(p, ih, iw, oh, ow)}")
                want = np_resize_planes(x, oh, ow, sy, sx, "linear", coord)
                assert_bits(run_kernel(ctx, x, oh, ow, sy, sx, "linear", coord, "floor"), want, f"linear {coord} {(p, ih, iw, oh, ow)}")
                assert_bits(run_kernel(ctx, x, oh, ow, sy, sx, "linear", coord, "floor", y_offset=1), want, f"linear unaligned {coord}")


def test_kernel_large_planes_and_unknown_modes(ctx):
    rng = np.random.default_rng(2)
    for (p, ih, iw, oh, ow), mode, coord in (((8 * 64, 40, 40, 80, 80), "nearest", "asymmetric"), ((2 * 64, 64, 64, 128, 128), "linear", "half_pixel"),
                                             ((2 * 21, 65, 65, 513, 513), "linear", "pytorch_half_pixel")):
        x = rng.standard_normal((p, ih, iw)).astype(np.float32)
        sy, sx = F(ih) / F(oh), F(iw) / F(ow)
        nearest = "floor" if mode == "nearest" else "round_prefer_floor"
        assert_bits(run_kernel(ctx, x, oh, ow, sy, sx, mode, coord, nearest), np_resize_planes(x, oh, ow, sy, sx, mode, coord, nearest), f"{mode} {p}x{oh}x{ow}")
    xd = DeviceTensor.from_numpy(ctx, np.zeros(16, np.float32))
    for m, c, n in ((2, 0, 0), (-1, 0, 0), (0, 4, 0), (1, -1, 0), (0, 0, 4), (1, 0, -1)):
        with pytest.raises(L.HipError) as e:
            ctx.call("rten_hip_resize_f32", m, c, n, 1, 2, 2, 4, 4, 0.5, 0.5, xd.vp, xd.vp)
        assert e.value.code == L.ERR_INVALID_VALUE, (m, c, n)


def test_operator_ranks_scales_sizes_and_quirks(ctx):
    rng = np.random.default_rng(3)
    cases = [((2, 3, 5, 7), dict(scales=[1, 1, 2, 2])), ((2, 3, 5, 7), dict(scales=[1, 1, 1.5, 0.6])), ((2, 3, 9, 4), dict(sizes=[2, 3, 4, 11])),
             ((2, 3, 7), dict(scales=[1, 1, 2.5])),       # 3-D NCW (tried before NHW)
             ((2, 6, 7), dict(sizes=[2, 3, 13])),         # 3-D NHW
             ((5, 9), dict(scales=[0.5, 3])), ((11,), dict(sizes=[4])), ((3,), dict(scales=[3]))]
    for shape, target in cases:
        x = with_specials(rng.standard_normal(shape).astype(np.float32), rng).reshape(shape)
        xd = DeviceTensor.from_numpy(ctx, x)
        for mode in ("nearest", "linear"):
            for coord in COORDS:
                op = ops.Resize(mode, coord, "round_prefer_ceil")
                s = np.array(target["scales"], np.float32) if "scales" in target else None
                z = np.array(target["sizes"], np.int32) if "sizes" in target else None
                got = op.run(ctx, [xd, None, s, z])[0]
                want = np_resize(x, s, z, mode, coord, "round_prefer_ceil")
                assert got.shape == want.shape, (shape, target)
                assert_bits(got.numpy(), want, f"{shape} {target} {mode} {coord}")
    x = rng.standard_normal((1, 2, 5, 5)).astype(np.float32)
    xd = DeviceTensor.from_numpy(ctx, x)
    # the same shape is a copy even though 1.1 is not 1 (floor(5 * 1.1) = 5): no resampling happens
    got = ops.Resize("linear").run(ctx, [xd, None, np.array([1, 1, 1.1, 1.1], np.float32)])[0].numpy()
    assert_bits(got, x, "same-shape copy")
    assert not np.array_equal(np_resize_planes(x.reshape(2, 5, 5), 5, 5, F(1) / F(1.1), F(1) / F(1.1), "linear").reshape(x.shape), x)
    # an empty output
    assert ops.Resize().run(ctx, [xd, None, np.array([1, 1, 0, 0], np.float32)])[0].shape == (1, 2, 0, 0)
    # align_corners with an output length of 1: 0 / 0 = NaN -> nearest reads index 0, linear gives NaN (here along the H axis of a W-only resize)
    x1 = rng.standard_normal((2, 3, 6)).astype(np.float32)
    x1d = DeviceTensor.from_numpy(ctx, x1)
    got = ops.Resize("linear", "align_corners").run(ctx, [x1d, None, np.array([1, 1, 2], np.float32)])[0].numpy()
    assert np.isnan(got).all() and got.shape == (2, 3, 12)
    got = ops.Resize("nearest", "align_corners").run(ctx, [x1d, None, None, np.array([2, 3, 1], np.int32)])[0].numpy()
    assert_bits(got, x1[:, :, :1], "align_corners nearest to length 1")
    # Upsample: asymmetric / floor, scales required
    for mode in ("nearest", "linear"):
        got = ops.Upsample(mode).run(ctx, [xd, np.array([1, 1, 2, 3], np.float32)])[0].numpy()
        assert_bits(got, np_resize(x, [1, 1, 2, 3], None, mode, "asymmetric", "floor"), f"Upsample {mode}")
    with pytest.raises(ops.OpError) as e:
        ops.Upsample().run(ctx, [xd])
    assert e.value == ops.MissingInputs


def test_split_operator(ctx):
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 7, 3, 5)).astype(np.float32)
    xd = DeviceTensor.from_numpy(ctx, x)
    for axis, kw, sizes, want_sizes in ((1, {}, [2, 0, 5], [2, 0, 5]), (-1, {"num_outputs": 2}, None, [3, 2]), (0, {"node_outputs": 2}, None, [1, 1]),
                                         (1, {"node_outputs": 3}, None, [3, 3, 1]), (1, {"node_outputs": 6}, None, [2, 2, 2, 1])):
        outs = ops.Split(axis, **kw).run(ctx, [xd] + ([np.array(sizes)] if sizes is not None else []))
        want = np.split(x, np.cumsum(want_sizes)[:-1], axis=axis)
        assert [o.shape for o in outs] == [w.shape for w in want], (axis, kw)
        for o, w in zip(outs, want):
            assert_bits(o.numpy(), w, f"split {axis} {kw}")
    xi = DeviceTensor.from_numpy(ctx, np.arange(24, dtype=np.int32).reshape(4, 6))
    outs = ops.Split(1).run(ctx, [xi, np.array([1, 5])])
    assert np.array_equal(outs[1].numpy(), np.arange(24, dtype=np.int32).reshape(4, 6)[:, 1:])


# ---------------------------------------------------------------------------------------------------- graphs
def run_graph(tmp_path, model_bytes, inputs, outs, *extra, batch=None):
    from tests.test_graph_executor import run_cli
    p = tmp_path / "m.onnx"
    p.write_bytes(model_bytes)
    args = []
    for name, arr in inputs.items():
        f = tmp_path / f"{name}.bin"
        arr.astype(np.float32).tofile(f)
        args += ["--input", f"{name}={f}"]
    for o in outs:
        args += ["--dump", f"{o}={tmp_path / (o + '.bin')}"]
    batch = batch if batch is not None else next(iter(inputs.values())).shape[0]
    r = run_cli("-s", f"batch={batch}", *args, *extra, str(p))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [np.fromfile(tmp_path / (o + ".bin"), np.float32) for o in outs], r.stdout


def test_torch_exported_yolo_network(tmp_path):
    """C2f (Split), SPPF, two nearest 2x Resize + Concat and a DFL head, exported by PyTorch, at batch 3: fused, unfused and replayed from a
    captured graph give the same bits; the -t table has Resize and Split steps; torch's CPU forward agrees to f32 accumulation-order tolerance."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export as te
    model = te.yolo_module()
    data = te.yolo_onnx(model)
    x = np.random.default_rng(5).standard_normal((3, 3, 64, 64)).astype(np.float32)
    (fused,), log = run_graph(tmp_path, data, {"x": x}, ["y"], "-t")
    (unfused,), _ = run_graph(tmp_path, data, {"x": x}, ["y"], "--no-fuse")
    (graph,), _ = run_graph(tmp_path, data, {"x": x}, ["y"], "--graph", "-n", "2")
    assert_bits(unfused, fused, "--no-fuse")
    assert_bits(graph, fused, "--graph")
    steps = [line.split() for line in log.splitlines()]
    assert any(s and s[0] == "Resize" for s in steps) and any(s and s[0] == "Split" for s in steps), log[-3000:]
    with torch.no_grad():
        want = model(torch.from_numpy(x)).numpy()
    np.testing.assert_allclose(fused.reshape(want.shape), want, rtol=1e-4, atol=1e-4)


def test_resize_forms_in_onnx_graphs(tmp_path):
    """Resize-11+ with roi = "" (scales) and sizes from a Shape subgraph under a dynamic batch; linear pytorch_half_pixel after a Conv with an
    empty roi / scales tensor (absent) and cubic (runs as linear); every result bit-exact against the oracle's convolution + the restatement."""
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, 3, 10, 14)).astype(np.float32)
    w = (rng.standard_normal((4, 3, 3, 3)) * 0.3).astype(np.float32)
    b = rng.standard_normal(4).astype(np.float32)
    scales = np.array([1, 1, 1.5, 2.5], np.float32)
    nodes = [ow.node("Resize", ["x", "", "scales"], ["y1"], name="rs_scales", mode="linear", coordinate_transformation_mode="asymmetric"),
             ow.node("Shape", ["x"], ["shp"], name="shape"),
             ow.node("Slice", ["shp", "s0", "s2"], ["nc"], name="nc"),
             ow.node("Concat", ["nc", "hw"], ["sizes"], name="sizes", axis=0),
             ow.node("Resize", ["x", "", "", "sizes"], ["y2"], name="rs_sizes"),
             ow.node("Conv", ["x", "w", "b"], ["c"], name="conv", kernel_shape=[3, 3], pads=[1, 1, 1, 1]),
             ow.node("Resize", ["c", "roi0", "scales0", "sizes3"], ["y3"], name="rs_conv", mode="linear", coordinate_transformation_mode="pytorch_half_pixel"),
             ow.node("Resize", ["c", "", "scales"], ["y4"], name="rs_cubic", mode="cubic", coordinate_transformation_mode="align_corners")]
    inits = [ow.tensor("scales", scales), ow.tensor("s0", np.array([0], np.int64)), ow.tensor("s2", np.array([2], np.int64)),
             ow.tensor("hw", np.array([7, 23], np.int64)), ow.tensor("w", w), ow.tensor("b", b), ow.tensor("roi0", np.zeros(0, np.float32)),
             ow.tensor("scales0", np.zeros(0, np.float32)), ow.tensor("sizes3", np.array([2, 4, 33, 19], np.int64))]
    outs = ["y1", "y2", "y3", "y4"]
    m = ow.model(nodes, [ow.value_info("x", ow.FLOAT, ["batch", 3, 10, 14])], [ow.value_info(o, ow.FLOAT, []) for o in outs], inits, opset=13)
    c = ref.conv2d_f32(x, w, b, pads=(1, 1, 1, 1))
    want = [np_resize(x, scales, None, "linear", "asymmetric"), np_resize(x, None, [2, 3, 7, 23]),
            np_resize(c, None, [2, 4, 33, 19], "linear", "pytorch_half_pixel"), np_resize(c, scales, None, "linear", "align_corners")]
    for extra in (("-t",), ("--no-fuse",), ("--graph", "-n", "2")):
        got, log = run_graph(tmp_path, m, {"x": x}, outs, *extra)
        for g, wv, o in zip(got, want, outs):
            assert_bits(g, wv, f"{o} {extra}")
    # the Shape-subgraph sizes alone at other batches: they follow the input's shape (the constant [2, 4, 33, 19] of y3 would change N at any
    # other batch, which the reference refuses as UnsupportedValue)
    m2 = ow.model(nodes[1:5], [ow.value_info("x", ow.FLOAT, ["batch", 3, 10, 14])], [ow.value_info("y2", ow.FLOAT, [])], inits, opset=13)
    for batch in (1, 5):
        xb = rng.standard_normal((batch, 3, 10, 14)).astype(np.float32)
        got, _ = run_graph(tmp_path, m2, {"x": xb}, ["y2"])
        assert_bits(got[0], np_resize(xb, None, [batch, 3, 7, 23]), f"y2 at batch {batch}")
    x5 = rng.standard_normal((5, 3, 10, 14)).astype(np.float32)
    from tests.test_graph_executor import run_cli
    p = tmp_path / "fixed.onnx"
    p.write_bytes(m)
    f = tmp_path / "x5.bin"
    x5.tofile(f)
    r = run_cli("-s", "batch=5", "--input", f"x={f}", str(p))
    assert r.returncode == 1 and "Only 1D to 4D inputs are supported with up to two resized dimensions" in r.stderr, r.stderr[-1000:]


def test_upsample_forms(tmp_path):
    """Upsample-7 (scales attribute) and Upsample-9 (scales input): asymmetric coordinates, floor."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, 3, 5, 6)).astype(np.float32)
    m7 = ow.model([ow.node("Upsample", ["x"], ["y"], name="up7", mode="nearest", scales=[1.0, 1.0, 2.0, 3.0])],
                  [ow.value_info("x", ow.FLOAT, ["batch", 3, 5, 6])], [ow.value_info("y", ow.FLOAT, [])], [], opset=7)
    (got,), _ = run_graph(tmp_path, m7, {"x": x}, ["y"])
    assert_bits(got, np_resize(x, [1, 1, 2, 3], None, "nearest", "asymmetric", "floor"), "Upsample-7")
    m9 = ow.model([ow.node("Upsample", ["x", "s"], ["y"], name="up9", mode="linear")], [ow.value_info("x", ow.FLOAT, ["batch", 3, 5, 6])],
                  [ow.value_info("y", ow.FLOAT, [])], [ow.tensor("s", np.array([1, 1, 2.5, 1.5], np.float32))], opset=9)
    (got,), _ = run_graph(tmp_path, m9, {"x": x}, ["y"])
    assert_bits(got, np_resize(x, [1, 1, 2.5, 1.5], None, "linear", "asymmetric", "floor"), "Upsample-9")


def test_split_forms(tmp_path):
    """Split-13 (sizes input), Split-18 (num_outputs), the output-count form and Split-11 (split attribute), after a Conv."""
    rng = np.random.default_rng(8)
    x = rng.standard_normal((2, 3, 9, 7)).astype(np.float32)
    w = (rng.standard_normal((6, 3, 1, 1)) * 0.5).astype(np.float32)
    c = ref.conv2d_f32(x, w, None)
    forms = [(13, dict(inputs=["c", "sp"], axis=1), [ow.tensor("sp", np.array([1, 3, 2], np.int64))], 3, [1, 3, 2], 1),
             (18, dict(inputs=["c"], axis=-1, num_outputs=3), [], 3, [3, 3, 1], 3),
             (13, dict(inputs=["c"], axis=2), [], 3, [3, 3, 3], 2),
             (11, dict(inputs=["c"], axis=1, split=[4, 2]), [], 2, [4, 2], 1)]
    for opset, attrs, extra_inits, n, sizes, axis in forms:
        attrs = dict(attrs)
        ins = attrs.pop("inputs")
        outs = [f"o{k}" for k in range(n)]
        m = ow.model([ow.node("Conv", ["x", "w"], ["c"], name="conv", kernel_shape=[1, 1]), ow.node("Split", ins, outs, name="split", **attrs)],
                     [ow.value_info("x", ow.FLOAT, ["batch", 3, 9, 7])], [ow.value_info(o, ow.FLOAT, []) for o in outs], [ow.tensor("w", w)] + extra_inits,
                     opset=opset)
        want = np.split(c, np.cumsum(sizes)[:-1], axis=axis)
        for extra in ((), ("--graph", "-n", "2")):
            got, _ = run_graph(tmp_path, m, {"x": x}, outs, *extra)
            for g, wv, o in zip(got, want, outs):
                assert_bits(g, wv, f"Split-{opset} {attrs} {o} {extra}")


def test_load_errors(tmp_path):
    from tests.test_graph_executor import run_cli
    for attrs, msg in ((dict(antialias=1), "must keep their defaults"), (dict(coordinate_transformation_mode="tf_crop_and_resize"), "tf_crop_and_resize"),
                       (dict(keep_aspect_ratio_policy="not_larger"), "must keep their defaults"), (dict(mode="bicubic"), "bicubic")):
        m = ow.model([ow.node("Resize", ["x", "", "s"], ["y"], name="rs", **attrs)], [ow.value_info("x", ow.FLOAT, [1, 1, 4, 4])],
                     [ow.value_info("y", ow.FLOAT, [])], [ow.tensor("s", np.array([1, 1, 2, 2], np.float32))], opset=13)
        p = tmp_path / "bad.onnx"
        p.write_bytes(m)
        r = run_cli(str(p))
        assert r.returncode != 0 and msg in r.stderr, (attrs, r.stdout[-500:], r.stderr[-500:])
