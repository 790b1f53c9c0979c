"""ReduceL1 / ReduceSumSquare / ReduceL2 / ReduceLogSum / ReduceLogSumExp / ReduceProd, LpNormalization and GlobalMaxPool on the GPU (rten_amd/csrc/reduce.hip
through rten_amd.ops and the graph executor).  Everything is compared bit for bit with the rules restated on the oracle (tests/reduce_rules.py); a NaN
result is compared as NaN.  The exported graphs are also held against torch's CPU forward within the bound the other exported-graph tests use
(tests/test_shape_arithmetic.py, tests/test_graph_executor.py: rtol = atol = 1e-4).

Before this family existed the loader refused tools/torch_export.embedding_head_onnx with GraphError "operator ReduceL2 is not available on the HIP backend
(no CPU fallback)": test_embedding_head_graph is the test that fails without it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from tests import confine as K
from tests import reduce_rules as R
from tests import select_rules
from tests.test_reduce_ops import OPS, prod_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32
pytestmark = pytest.mark.gpu
# 5 slices (not a multiple of the four slices per wave) of every length around a dispatch boundary or a tail form: n % 64, n % 16, fewer than 16
LENGTHS = [1, 15, 16, 17, 63, 64, 65, 128, 129, 256, 257, 1000, 4100]
TORCH_TOL = dict(rtol=1e-4, atol=1e-4)


def i64(v):
    return (C.c_int64 * max(len(v), 1))(*[int(a) for a in v])


def dev(ctx, a):
    from rten_amd.tensor import DeviceTensor
    a = np.asarray(a)
    return DeviceTensor.from_numpy(ctx, a if a.ndim == 0 else np.ascontiguousarray(a))  # (ascontiguousarray would turn a 0-d scalar into shape [1])


def data(kind, shape, seed):
    """Operands under which every kind has something to say: values of both signs; ReduceLogSum gets positive sums, ReduceProd factors near 1 (4100 of them
    neither overflow nor vanish)."""
    r = np.random.default_rng(seed).standard_normal(shape)
    if kind == "prod":
        return (1 + r * 1e-2).astype(F)
    if kind == "log_sum":
        return (np.abs(r) + 0.05).astype(F)
    return (r * 3).astype(F)


def run(ctx, kind, x, axes=None, keep=True, noop=False):
    return OPS[kind](axes=axes, keep_dims=keep, noop_with_empty_axes=noop).run(ctx, [x if not isinstance(x, np.ndarray) else dev(ctx, x)])[0].numpy()


# ================================================================================================ every kind x slice length
@pytest.mark.parametrize("kind", R.KINDS)
def test_every_kind_and_slice_length(ctx, kind):
    lengths = LENGTHS + ([1024, 1025] if kind == "log_sum_exp" else [])  # the register / two-pass boundary of ReduceLogSumExp, both sides
    for n in lengths:
        x = data(kind, (5, n), 100 + n)
        R.same_bits(run(ctx, kind, x, [1], False), R.reduce(kind, x, [1], False), f"{kind} [5, {n}]")


# ================================================================================================ column form
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", [(70, 37), (300, 16)])
def test_column_form(ctx, kind, shape):
    """Reduced axis strided and longer than 64, kept axis contiguous, last dim not a multiple of 16 / exactly one group."""
    x = data(kind, shape, 7)
    R.same_bits(run(ctx, kind, x, [0], False), R.reduce(kind, x, [0], False), f"{kind} {shape} axis 0")
    R.same_bits(run(ctx, kind, x, [0], True), R.reduce(kind, x, [0], True), f"{kind} {shape} axis 0 keepdims")


# ================================================================================================ generic walk
@pytest.mark.parametrize("kind", R.KINDS)
def test_generic_walk_and_views(ctx, kind):
    from rten_amd import einsum as E
    x = data(kind, (3, 5, 4, 6), 11)
    for axes in ([1, 3], None, [0, 1, 2, 3], [-1, 1, 1]):
        for keep in (True, False):
            R.same_bits(run(ctx, kind, x, axes, keep), R.reduce(kind, x, axes, keep), f"{kind} axes {axes} keepdims {keep}")
    t = dev(ctx, x)
    base = K.dense(x.shape)
    perm = (2, 0, 3, 1)
    tv = E.View(t, [x.shape[p] for p in perm], [base[p] for p in perm])  # a Transpose that was never materialised
    for axes in ([1, 3], [0], [2]):
        R.same_bits(run(ctx, kind, tv, axes, False), R.reduce(kind, x.transpose(perm), axes, False), f"{kind} transposed view axes {axes}")
    sv = E.View(t, [3, 5, 4, 3], [base[0], base[1], base[2], 2])  # every second element of the last axis
    for axes in ([3], [1, 3], [0, 2]):
        R.same_bits(run(ctx, kind, sv, axes, True), R.reduce(kind, x[..., ::2], axes, True), f"{kind} step-2 view axes {axes}")


# ================================================================================================ ReduceLogSumExp
def test_log_sum_exp_special_rows(ctx):
    inf, nan = np.inf, np.nan
    for n in (7, 70, 300, 1024, 1025, 1100):
        x = data("log_sum_exp", (9, n), n)
        x[0, n // 2] = inf                      # +inf: the result is +inf
        x[1, :] = -inf                          # -inf only: -inf
        x[2, n - 1] = nan                       # a NaN anywhere: NaN
        x[3, 0], x[3, n - 1] = 1e4, -1e4        # exp(1e4) overflows without the max subtracted
        x[4, :] = 2.5                           # equal values: 2.5 + ln(n)
        x[5, 0], x[5, 1:] = 3.0, -inf           # -inf among finite values: exp gives 0
        x[6, :] = -1e4                          # far below exp's range until the max is subtracted
        x[7, n // 3] = nan
        x[7, 0] = inf                           # NaN wins over inf
        got, want = run(ctx, "log_sum_exp", x, [1], False), R.reduce("log_sum_exp", x, [1], False)
        R.same_bits(got, want, f"log_sum_exp specials n {n}")
        assert got[0] == inf and got[1] == -inf and np.isnan(got[2]) and np.isfinite(got[3]) and np.isnan(got[7])
        assert got[4] == R.F(F(2.5) + R.ln(R.sum_exp_sub(x[4], 2.5)))


# ================================================================================================ ReduceProd
def test_prod_special_rows_and_order(ctx):
    row = prod_row()
    assert R.prod(row).view(np.uint32) != R.pairwise_prod(row).view(np.uint32)  # (otherwise the row shows nothing about the order)
    x = np.tile(row, (6, 1))
    x[1, 100] = 0.0                                   # a zero
    x[2, :3] = [1e-20, 1e-20, 1e10]                   # the chain passes through a subnormal (1e-40) and comes back
    x[3, :4] = [3e38, 10.0, 1e-30, 1e-30]             # overflows to inf, then stays
    x[4, :3] = [3e38, 10.0, 0.0]                      # inf * 0 = NaN
    x[5, 200] = -0.0
    got, want = run(ctx, "prod", x, [1], False), R.reduce("prod", x, [1], False)
    R.same_bits(got, want, "prod specials")
    assert got[0].view(np.uint32) == R.prod(row).view(np.uint32) and got[1] == 0 and np.isinf(got[3]) and np.isnan(got[4])
    # the same chains when the slices lie along a strided axis (the column form), and for 70 slices (two workgroups of 64)
    xt = np.ascontiguousarray(np.tile(row[:, None], (1, 70)))
    R.same_bits(run(ctx, "prod", xt, [0], False), np.full(70, R.prod(row), F), "prod columns")
    xr = np.tile(row, (70, 1))
    R.same_bits(run(ctx, "prod", xr, [1], False), np.full(70, R.prod(row), F), "prod 70 rows")


# ================================================================================================ int32
@pytest.mark.parametrize("kind", R.INT32_KINDS)
def test_int32_wraps(ctx, kind):
    rng = np.random.default_rng(5)
    for shape, axes in (((5, 257), [1]), ((70, 37), [0]), ((3, 5, 4, 6), [1, 3]), ((3, 5, 4, 6), None)):
        x = rng.integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)  # full range: every sum and product wraps
        if kind == "prod":
            x |= 1  # odd factors: the product never collapses to 0
        R.same_bits(run(ctx, kind, x, axes, False), R.reduce(kind, x, axes, False), f"int32 {kind} {shape} axes {axes}")
    edge = np.array([[2**31 - 1, 1, -2**31], [65536, 65536, 3], [-2**31, -1, 1]], np.int32)
    R.same_bits(run(ctx, kind, edge, [1], True), R.reduce(kind, edge, [1], True), f"int32 {kind} edges")


# ================================================================================================ empty slices, 0-d input, noop_with_empty_axes
@pytest.mark.parametrize("kind", R.KINDS)
def test_empty_zero_d_and_noop(ctx, kind):
    dtypes = [np.float32] + ([np.int32] if kind in R.INT32_KINDS else [])
    for dt in dtypes:
        e = np.zeros((3, 0, 5), dt)
        R.same_bits(run(ctx, kind, e, [1], False), R.reduce(kind, e, [1], False), f"{kind} empty slices")
        R.same_bits(run(ctx, kind, e, [1], True), R.reduce(kind, e, [1], True), f"{kind} empty slices keepdims")
        assert run(ctx, kind, e, [0], False).shape == (0, 5)
        s = np.array(-3 if dt == np.int32 else -2.5, dt)
        R.same_bits(run(ctx, kind, s), R.reduce(kind, s), f"{kind} 0-d")
        x = data(kind, (4, 9), 3) if dt == np.float32 else np.random.default_rng(3).integers(-2**31, 2**31, (4, 9), np.int64).astype(np.int32)
        if kind == "log_sum":
            x[0, :3] = [0.0, -1.0, np.inf]  # ln(0) = -inf, ln(-1) = NaN
        for axes in (None, []):
            R.same_bits(run(ctx, kind, x, axes, True, noop=True), R.reduce(kind, x, axes, True, True), f"{kind} noop_with_empty_axes")


# ================================================================================================ LpNormalization
def lp(ctx, x, axis, p):
    from rten_amd import ops
    return ops.LpNormalization(axis=axis, p=p).run(ctx, [dev(ctx, x)])[0].numpy()


@pytest.mark.parametrize("p", [1, 2])
def test_lp_normalization_lengths(ctx, p):
    # LENGTHS, and both sides of every register-form boundary and of the register / streaming boundary
    for n in LENGTHS + [512, 513, 768, 769, 1024, 1025]:
        x = data("l2", (5, n), 200 + n)
        R.same_bits(lp(ctx, x, -1, p), R.lp_normalization(x, -1, p), f"lp p {p} [5, {n}]")


@pytest.mark.parametrize("p", [1, 2])
def test_lp_normalization_special_lanes_and_axes(ctx, p):
    x = data("l2", (6, 40), 9)
    x[1, :] = 0.0                                   # a zero lane stays zero (not NaN)
    x[2, :] = 0.0
    x[2, 3] = 1e-42                                 # p = 1: a subnormal norm, 1 / norm = inf: inf at 3, 0 * inf = NaN elsewhere; p = 2: the square underflows, a zero lane
    x[3, 5] = np.nan
    x[4, 7] = np.inf
    got, want = lp(ctx, x, 1, p), R.lp_normalization(x, 1, p)
    R.same_bits(got, want, f"lp p {p} specials")
    assert not got[1].any() and np.isnan(got[3]).all()
    assert (np.isinf(got[2, 3]) and np.isnan(got[2, 0])) if p == 1 else not got[2].any()
    y = data("l2", (70, 37), 10)                    # axis 0: lanes strided by 37, 37 lanes
    R.same_bits(lp(ctx, y, 0, p), R.lp_normalization(y, 0, p), f"lp p {p} axis 0 of [70, 37]")
    z = data("l2", (3, 5, 4, 6), 11)
    for axis in (0, 1, 2, 3, -2):
        R.same_bits(lp(ctx, z, axis, p), R.lp_normalization(z, axis, p), f"lp p {p} axis {axis}")
    assert lp(ctx, np.zeros((3, 0, 2), F), 1, p).shape == (3, 0, 2)


@pytest.mark.parametrize("n", [100, 1024, 1500])
def test_lp_normalization_in_place(ctx, n):
    """The entry point allows y == x: a wave reads its whole lane (or finishes its reduction) before it stores."""
    x = data("l2", (7, n), n)
    for p in (1, 2):
        t = dev(ctx, x)
        ctx.call("rten_hip_lp_normalize_f32", p, 1, i64([7]), i64([n]), n, 1, t.vp, t.vp)
        R.same_bits(t.numpy(), R.lp_normalization(x, -1, p), f"lp in place p {p} n {n}")


# ================================================================================================ GlobalMaxPool
def test_global_max_pool(ctx):
    from rten_amd import ops
    for shape in ((2, 3, 5, 7), (2, 3, 9), (2, 3)):
        x = data("l2", shape, 13)
        got = ops.GlobalMaxPool().run(ctx, [dev(ctx, x)])[0].numpy()
        assert got.shape == shape[:2] + (1,) * (len(shape) - 2)
        R.same_bits(got, R.global_max_pool(x), f"global max pool {shape}")
    x = data("l2", (2, 3, 5, 7), 14)
    x[0, 1, 2, 3] = np.nan                           # a NaN inside: that plane is NaN, no other
    x[1, 0] = -1.0
    x[1, 0, 0, 0], x[1, 0, 4, 6] = -0.0, 0.0         # a +-0 tie at the maximum
    got = ops.GlobalMaxPool().run(ctx, [dev(ctx, x)])[0].numpy()
    want = R.global_max_pool(x)
    assert np.array_equal(select_rules.canon(got, True), select_rules.canon(want, True)), (got, want)  # (the sign of a zero maximum is not part of the contract)
    assert np.isnan(got[0, 1, 0, 0]) and np.isfinite(np.delete(got.reshape(-1), 1)).all() and got[1, 0, 0, 0] == 0


# ================================================================================================ confinement
def guarded_call(ctx, what, x, want, call, out_shape=None, out_strides=None, leads=(0, 1, 3)):
    """`call(x pointer, y pointer)` with x and a guarded y `lead` elements off a 16-byte boundary: y holds `want` at out_shape / out_strides and nothing
    else of the allocation has changed."""
    out_shape = want.shape if out_shape is None else out_shape
    out_strides = K.dense(want.shape) if out_strides is None else out_strides
    for lead in leads:
        xg = K.Guarded(ctx, x, lead=lead)
        out = K.Guarded(ctx, K.span(out_shape, out_strides) * want.dtype.itemsize, lead=lead, itemsize=want.dtype.itemsize)
        call(xg.vp, out.vp)
        ctx.sync()
        w = f"{what} lead {lead}"
        R.same_bits(out.check(out.raw(), out_shape, out_strides, want.dtype, w), want, w)


@pytest.mark.parametrize("e", [1, 3, 5, 67])
def test_reduce_strided_writes_its_output_only(ctx, e):
    from rten_amd import lib as L
    x = K.seeded((3, 5, e), 55, 8.0)
    last = dict(osh=(3, 5), ost=(5 * e, e), ish=(e,), ist=(1,), axes=[2])   # over the innermost axis
    mid = dict(osh=(3, e), ost=(5 * e, 1), ish=(5,), ist=(e,), axes=[1])    # over the middle axis: the output's innermost extent is e
    for g in (last, mid):
        for code, kind in enumerate(R.KINDS):
            xk = np.abs(x) + F(0.25) if kind == "log_sum" else x
            guarded_call(ctx, f"reduce_strided {kind} axes {g['axes']} e {e}", xk, R.reduce(kind, xk, g["axes"], False),
                         lambda xv, yv: ctx.call("rten_hip_reduce_strided", code, L.DT_F32, 2, i64(g["osh"]), i64(g["ost"]), 1, i64(g["ish"]), i64(g["ist"]), xv, yv))
        xi = (x * 1e8).astype(np.int32)
        for kind in R.INT32_KINDS:
            guarded_call(ctx, f"reduce_strided int32 {kind} axes {g['axes']} e {e}", xi, R.reduce(kind, xi, g["axes"], False),
                         lambda xv, yv: ctx.call("rten_hip_reduce_strided", R.KINDS.index(kind), L.DT_I32, 2, i64(g["osh"]), i64(g["ost"]), 1, i64(g["ish"]), i64(g["ist"]), xv, yv))


@pytest.mark.parametrize("e", [1, 3, 5, 67, 1100])
def test_lp_normalize_writes_its_output_only(ctx, e):
    """Contiguous lanes, lanes along a strided axis, and rows placed with slack between them (a row stride above the lane length): the gaps keep their fill."""
    rows = 3
    x = K.seeded((rows, 5, e), 56, 4.0)
    for p in (1, 2):
        guarded_call(ctx, f"lp_normalize p {p} last axis e {e}", x, R.lp_normalization(x, -1, p),
                     lambda xv, yv: ctx.call("rten_hip_lp_normalize_f32", p, 1, i64([rows * 5]), i64([e]), e, 1, xv, yv))
        if e <= 67:
            guarded_call(ctx, f"lp_normalize p {p} middle axis e {e}", x, R.lp_normalization(x, 1, p),
                         lambda xv, yv: ctx.call("rten_hip_lp_normalize_f32", p, 2, i64([rows, e]), i64([5 * e, 1]), 5, e, xv, yv))
        # 4 lanes of e elements, e + 3 apart, in x and in y
        pitch = e + 3
        padded = np.full((4, pitch), np.nan, F)
        padded[:, :e] = K.seeded((4, e), 57, 4.0)
        want = R.lp_normalization(padded[:, :e], -1, p)
        guarded_call(ctx, f"lp_normalize p {p} pitched rows e {e}", padded, want,
                     lambda xv, yv: ctx.call("rten_hip_lp_normalize_f32", p, 1, i64([4]), i64([pitch]), e, 1, xv, yv), out_shape=(4, e), out_strides=(pitch, 1))


@pytest.mark.parametrize("cols", [17, 257, 1100])
def test_non_finite_operands_stay_in_their_slice(ctx, cols):
    """A NaN / Inf in one slice leaves every other slice's result unchanged (bit for bit what the clean input gives)."""
    clean = K.seeded((20, cols), 58, 4.0)  # (20 slices: transposed, the kept axis is long enough for the column forms)
    dirty, dep = K.rows_nonfinite(clean)
    for kind in R.KINDS:
        c = (np.abs(clean) + F(0.25)) if kind == "log_sum" else clean
        d = c.copy()
        d[~np.isfinite(dirty)] = dirty[~np.isfinite(dirty)]
        got_clean, got_dirty = run(ctx, kind, c, [1], False), run(ctx, kind, d, [1], False)
        R.same_bits(got_dirty, R.reduce(kind, d, [1], False), f"{kind} non-finite cols {cols}")
        assert np.array_equal(got_clean[~dep].view(np.uint32), got_dirty[~dep].view(np.uint32)), kind
        # ... and along a strided axis (the column forms): slices are columns
        gt_clean, gt_dirty = run(ctx, kind, np.ascontiguousarray(c.T), [0], False), run(ctx, kind, np.ascontiguousarray(d.T), [0], False)
        R.same_bits(gt_dirty, R.reduce(kind, np.ascontiguousarray(d.T), [0], False), f"{kind} non-finite columns {cols}")
        assert np.array_equal(gt_clean[~dep].view(np.uint32), gt_dirty[~dep].view(np.uint32)), kind
    for p in (1, 2):
        got_clean, got_dirty = lp(ctx, clean, -1, p), lp(ctx, dirty, -1, p)
        R.same_bits(got_dirty, R.lp_normalization(dirty, -1, p), f"lp p {p} non-finite cols {cols}")
        assert np.array_equal(got_clean[~dep].view(np.uint32), got_dirty[~dep].view(np.uint32))


# ================================================================================================ graphs
MODES = (("-t",), (), ("--no-fuse",), ("--graph",))  # node by node (a sync after every step), fused, unfused, captured into a hipGraph and replayed


def clip_min(x, lo):
    """Clip(min = lo), max absent (the generic Clamp of the reference: `x > lo ? x : lo`)."""
    return np.where(x > F(lo), x, F(lo)).astype(F)


def embedding_rules(cfg, w, ids, mask, tts, p):
    """The head's nodes, one rounded float32 operation each, on the oracle's encoder: Mul by the mask, ReduceSum over the tokens, Clip, Div, ReduceL2 /
    ReduceL1 (keepdims), Clip, Expand, Div."""
    from oracle import einsum as oe
    from oracle import models as om
    B, S = ids.shape
    h = om.bert_forward(cfg, w, ids, mask, tts).reshape(B, S, -1)
    m = mask.astype(F)[:, :, None]
    pooled = (oe.reduce_sum((h * m).astype(F), [1]) / clip_min(oe.reduce_sum(m, [1]), 1e-9)).astype(F)
    norm = R.reduce("l2" if p == 2 else "l1", pooled, [1], True)
    return (pooled / np.broadcast_to(clip_min(norm, 1e-12), pooled.shape)).astype(F)


def run_graph(tmp_path, model_path, inputs, outputs, sizes, extra):
    from tests.test_graph_executor import run_cli
    args = list(extra)
    for k, v in sizes.items():
        args += ["-s", f"{k}={v}"]
    for name, arr in inputs.items():
        arr.tofile(tmp_path / (name + ".bin"))
        args += ["--input", f"{name}={tmp_path / (name + '.bin')}"]
    for name in outputs:
        args += ["--dump", f"{name}={tmp_path / (name + '.out')}"]
    r = run_cli(*args, str(model_path))
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2500:]
    return {name: np.fromfile(tmp_path / (name + ".out"), F) for name in outputs}, r.stdout


@pytest.mark.parametrize("form", ["static-l2", "static-l1", "dynamic-l2"])
def test_embedding_head_graph(tmp_path, form):
    """tools/torch_export.embedding_head_onnx (hidden 32, 2 heads, 2 layers; masked mean pooling; F.normalize) loads with no refused node and gives the
    rules' embedding bit for bit in all four run modes; with dynamic axes the same file runs at (2, 5) and (3, 7)."""
    import torch
    import torch_export as te
    from rten_amd.workloads import bert
    dynamic, p = form.startswith("dynamic"), 1 if form.endswith("l1") else 2
    cfg = te.embedding_head_config()
    w = bert.make_weights(cfg)
    path = tmp_path / "embedding_head.onnx"
    path.write_bytes(te.embedding_head_onnx(te.embedding_head_module(cfg, w, 5, float(p), dynamic), 2, 5, dynamic))
    rng = np.random.default_rng(5)
    for (B, S) in ((2, 5), (3, 7)) if dynamic else ((2, 5),):
        ids = rng.integers(0, cfg.vocab, (B, S)).astype(np.int32)
        tts = rng.integers(0, 2, (B, S)).astype(np.int32)
        mask = np.ones((B, S), np.int32)
        mask[1, S - 2:] = 0
        want = embedding_rules(cfg, w, ids, mask, tts, p)
        for extra in MODES:
            got, log = run_graph(tmp_path, path, {"input_ids": ids, "token_type_ids": tts, "attention_mask": mask}, ["embedding"],
                                 {"batch": B, "seq": S} if dynamic else {}, extra)
            R.same_bits(got["embedding"].reshape(want.shape), want, f"embedding head {form} ({B}, {S}) {extra}")
            if extra == ("-t",):
                assert ("ReduceL2" if p == 2 else "ReduceL1") in log, log[-2500:]
        with torch.no_grad():
            t = te.embedding_head_module(cfg, w, S, float(p), dynamic)(torch.from_numpy(ids.astype(np.int64)), torch.from_numpy(mask.astype(np.int64)),
                                                                        torch.from_numpy(tts.astype(np.int64))).numpy()
        np.testing.assert_allclose(got["embedding"].reshape(t.shape), t, **TORCH_TOL)
        np.testing.assert_allclose(np.abs(want).sum(1) if p == 1 else np.sqrt((want.astype(np.float64) ** 2).sum(1)), 1.0, rtol=1e-5)  # it IS normalised


def test_reduce_zoo_graph(tmp_path):
    """F.normalize(p = 1), logsumexp, a two-axis vector_norm, prod and (x * x).sum as PyTorch's exporter writes them, dynamic batch, at two batch sizes."""
    import torch
    import torch_export as te
    from oracle import einsum as oe
    path = tmp_path / "reduce_zoo.onnx"
    path.write_bytes(te.reduce_zoo_onnx())
    for B in (2, 3):
        x = (np.random.default_rng(B).standard_normal((B, 3, 4, 6)) * 1.5).astype(F)
        l1 = R.reduce("l1", x, [-1], True)
        want = {"l1_normalized": (x / np.broadcast_to(clip_min(l1, 1e-12), x.shape)).astype(F), "logsumexp": R.reduce("log_sum_exp", x, [2], False),
                "norm2": R.reduce("l2", x, [1, 2], False), "prod": R.reduce("prod", x, [1], False), "sum_of_squares": oe.reduce_sum((x * x).astype(F), [3])}
        for extra in MODES:
            got, _ = run_graph(tmp_path, path, {"x": x}, te.ZOO_OUTPUTS, {"batch": B}, extra)
            for name in te.ZOO_OUTPUTS:
                R.same_bits(got[name].reshape(want[name].shape), want[name], f"reduce zoo {name} batch {B} {extra}")
        with torch.no_grad():
            t = te.reduce_zoo_module()(torch.from_numpy(x))
        for name, tv in zip(te.ZOO_OUTPUTS, t):
            np.testing.assert_allclose(got[name].reshape(tv.shape), tv.numpy(), **TORCH_TOL)


def test_hand_built_reduce_family_graph(tmp_path):
    """rten_amd.onnx_writer.reduce_family_graph: LpNormalization (both p, a non-last axis), GlobalMaxPool, ReduceLogSum, ReduceSumSquare and two Reduce
    nodes with noop_with_empty_axes = 1 -- the nodes PyTorch's exporter never writes."""
    from rten_amd import onnx_writer as ow
    path = tmp_path / "reduce_family.onnx"
    path.write_bytes(ow.reduce_family_graph())
    for B in (2, 3):
        x = (np.random.default_rng(20 + B).standard_normal((B, 3, 5, 7)) * 2).astype(F)
        x[0, 1, :, :] = 0  # a zero lane for lp1_last, zeros for lp2_channels
        want = {"lp2_channels": R.lp_normalization(x, 1, 2), "lp1_last": R.lp_normalization(x, -1, 1), "global_max": R.global_max_pool(x),
                "log_sum": R.reduce("log_sum", (np.abs(x) + F(1)).astype(F), [2, 3], False), "sum_square": R.reduce("sum_square", x, [-1], True),
                "l1_noop": R.reduce("l1", x, None, True, True), "log_sum_exp_noop": R.reduce("log_sum_exp", x, [], True, True)}
        for extra in MODES:
            got, _ = run_graph(tmp_path, path, {"x": x}, ow.REDUCE_FAMILY_OUTPUTS, {"batch": B}, extra)
            for name in ow.REDUCE_FAMILY_OUTPUTS:
                g, wv = got[name].reshape(want[name].shape), want[name]
                if name == "global_max":  # (the sign of a zero maximum is not part of the contract)
                    assert np.array_equal(select_rules.canon(g, True), select_rules.canon(wv, True)), (name, extra)
                else:
                    R.same_bits(g, wv, f"reduce family {name} batch {B} {extra}")
