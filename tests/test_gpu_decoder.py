"""RMSNormalization / SimplifiedLayerNormalization, the skip forms and the two RotaryEmbedding operators on the device (rten_amd/csrc/decoder.hip): the three
entry points bit for bit against tests/decoder_rules.py on guarded, misaligned operands -- every form boundary of the launch rule, the row counts around a
workgroup's share, both scale forms, aliasing, non-finite and out-of-range rows; rotary in both layouts, both pairings, every cache and position form and a
q block read in place -- then the Python operators, and onnx_writer.norm_rotary_graph / decoder_block_graph through the CLI and the C-ABI model (eager,
captured, unfused)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import confine as K
from tests import decoder_rules as R
from tests.reduce_rules import RuleError, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
pytestmark = pytest.mark.gpu

LAYER, RMS = 0, 1
# the launch rule of rten_amd/csrc/decoder.hip: 16-byte groups per thread double at 256 / 512 (one wave per row), a workgroup per row above 1024 with
# groups doubling at 2048 / 4096, two passes above 8192.  It has no row-count term: a workgroup takes 4 rows up to 1024 columns and 1 row above.
BOUNDARIES = [256, 512, 1024, 2048, 4096, 8192]
COLS = sorted({1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 8192, 8193, 8275} | {t + d for t in BOUNDARIES for d in (-1, 0, 1)})
ROWS = [1, 3, 5]  # 5: one more than the four rows of a workgroup (up to 1024 columns); 3: more than the one row of a workgroup above that


def noise(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


_WANT = {}


def want_rms(x, gamma, gs, eps):
    """The rule's rows, computed once per (input, scale) and shared (the fold is a Python loop)."""
    key = (x.tobytes(), None if gamma is None else gamma.tobytes(), gs, eps)
    if key not in _WANT:
        _WANT[key] = np.stack([R.rms_row(r, gamma, gs, eps) for r in x]) if x.shape[0] else x.copy()
    return _WANT[key]


def rms_norm(ctx, x, gamma, gs=1.0, eps=1e-5, leads=(0, 0, 0), alias=False, what=""):
    """rten_hip_rms_norm_f32 on guarded operands `lead` elements off a 16-byte boundary -> y, confined and bit-equal to the rule."""
    rows, cols = x.shape
    xg = K.Guarded(ctx, x, lead=leads[0])
    gg = K.Guarded(ctx, gamma, lead=leads[1]) if gamma is not None else None
    yg = xg if alias else K.Guarded(ctx, x.nbytes, lead=leads[2])
    ctx.call("rten_hip_rms_norm_f32", rows, cols, xg.vp, gg.vp if gg else None, gs, eps, yg.vp)
    what = f"rms_norm {what} rows {rows} cols {cols} gamma {'vector' if gamma is not None else gs} leads {leads} alias {alias}"
    got = yg.check(yg.raw(), x.shape, K.dense(x.shape), F, what)
    if not alias:
        xg.check(xg.raw(), x.shape, K.dense(x.shape), F, what + " (the input)")
    same_bits(got, want_rms(x, gamma, gs, eps), what)
    return got


def skip_norm(ctx, mode, x, skip, gamma, beta=None, bias=None, eps=1e-5, with_sum=True, leads=(0, 0, 0, 0), alias=None, what=""):
    """rten_hip_skip_norm_f32 -> (y, sum); x is [rows, cols], skip [skip_rows, cols].  alias: None, "y=x", "sum=x", "y=skip"."""
    rows, cols = x.shape
    xg, sg = K.Guarded(ctx, x, lead=leads[0]), K.Guarded(ctx, skip, lead=leads[1])
    gg = K.Guarded(ctx, gamma, lead=leads[1])
    bg = K.Guarded(ctx, beta, lead=leads[0]) if beta is not None else None
    ag = K.Guarded(ctx, bias, lead=leads[2]) if bias is not None else None
    yg = xg if alias == "y=x" else sg if alias == "y=skip" else K.Guarded(ctx, x.nbytes, lead=leads[2])
    tg = (xg if alias == "sum=x" else K.Guarded(ctx, x.nbytes, lead=leads[3])) if with_sum else None
    ctx.call("rten_hip_skip_norm_f32", mode, rows, cols, xg.vp, sg.vp, skip.shape[0], ag.vp if ag else None, gg.vp, bg.vp if bg else None, eps,
             tg.vp if tg else None, yg.vp)
    what = f"skip_norm {what} mode {mode} rows {rows} skip_rows {skip.shape[0]} cols {cols} beta {beta is not None} bias {bias is not None} sum {with_sum} " \
           f"leads {leads} alias {alias}"
    got = yg.check(yg.raw(), x.shape, K.dense(x.shape), F, what)
    total = tg.check(tg.raw(), x.shape, K.dense(x.shape), F, what + " (sum_out)") if tg else None
    full_skip = np.tile(skip, (rows // skip.shape[0], 1))
    with np.errstate(all="ignore"):
        t = (x + full_skip).astype(F)
        if bias is not None:
            t = (t + bias).astype(F)
    want = want_rms(t, gamma, 1.0, eps) if mode == RMS else R.layer_normalization_last(t, gamma, beta, eps)
    same_bits(got, want, what)
    if total is not None:
        same_bits(total, t, what + " (sum_out)")
    return got, total


# ================================================================================================ RMS normalisation
@pytest.mark.parametrize("cols", COLS)
def test_rms_norm_every_form_and_row_count_both_scale_forms(ctx, cols):
    gamma = noise(cols, cols)
    for rows in ROWS:
        x = noise(1000 * rows + cols, rows, cols)
        x[0, 0] = -0.0  # a -0 product: +0 behind the one-element scale's mul_add, -0 behind the per-element multiply
        rms_norm(ctx, x, gamma)
        got = rms_norm(ctx, x, None, gs=0.75, eps=1e-6)
        assert not np.signbit(got[0, 0])
    x = noise(cols, 2, cols)
    rms_norm(ctx, x, gamma, leads=(1, 2, 3), what="misaligned")
    rms_norm(ctx, x, gamma, alias=cols <= 8192, what="in place")


def test_rms_norm_rows_with_nan_inf_overflow_and_subnormals(ctx):
    from tests import range_cases as RC
    for cols in (200, 4096):
        x = noise(cols, 7, cols)
        x[1, cols // 2] = np.nan
        x[2, 3] = np.inf
        x[3, -1] = -np.inf
        x[4, 5] = 1e20   # x * x overflows: r = 0, the row is zeros
        x[5] = RC.wide(np.random.default_rng(cols), (cols,), -140, -127)  # subnormals
        gamma = noise(1, cols)
        got = rms_norm(ctx, x, gamma, what="non-finite")
        assert np.isnan(got[1]).all() and not got[4].any() and np.isnan(got[2, 3]) and not np.delete(got[2], 3).any()
        assert np.isfinite(got[[0, 5, 6]]).all()
        rms_norm(ctx, x, None, gs=1.0, what="non-finite, one-element scale")


# ================================================================================================ the skip forms
@pytest.mark.parametrize("cols", [1, 17, 64, 255, 256, 257, 1023, 1024, 1025, 2049, 4096, 4097, 8192, 8193])
@pytest.mark.parametrize("mode", [LAYER, RMS])
def test_skip_norm_forms_with_and_without_bias_beta_and_sum(ctx, mode, cols):
    gamma, beta, bias = noise(1, cols), noise(2, cols), noise(3, cols)
    for rows in ROWS if cols <= 1025 else [1, 3]:
        x, skip = noise(rows + cols, rows, cols), noise(rows + cols + 1, rows, cols)
        skip_norm(ctx, mode, x, skip, gamma, beta if mode == LAYER else None, bias)
        skip_norm(ctx, mode, x, skip, gamma, None, None, with_sum=False, leads=(1, 2, 3, 1), what="misaligned")
    x, skip = noise(cols, 6, cols), noise(cols + 1, 3, cols)
    skip_norm(ctx, mode, x, skip, gamma, None, bias, what="skip broadcast over the batch")
    if cols <= 8192:
        skip_norm(ctx, mode, x[:3], skip, gamma, None, None, alias="y=x", what="in place")
        skip_norm(ctx, mode, x[:3], skip, gamma, None, bias, alias="sum=x", what="residual stream in place")
        skip_norm(ctx, mode, x[:3], skip, gamma, None, None, with_sum=False, alias="y=skip", what="over the skip")


def test_skip_norm_refuses_what_it_does_not_cover(ctx):
    from rten_amd import lib as L
    x, y = K.Guarded(ctx, noise(1, 4, 8)), K.Guarded(ctx, 4 * 8 * 4)
    g = K.Guarded(ctx, noise(2, 8))
    for args in ((2, 4, 8, x.vp, x.vp, 4, None, g.vp, None), (RMS, 4, 8, x.vp, None, 4, None, g.vp, None), (RMS, 4, 8, x.vp, x.vp, 3, None, g.vp, None),
                 (RMS, 4, 8, x.vp, x.vp, 4, None, g.vp, g.vp), (RMS, 4, 8, x.vp, x.vp, 4, None, None, None)):
        with pytest.raises(L.HipError):
            ctx.call("rten_hip_skip_norm_f32", *args, 1e-5, None, y.vp)
    y.check(y.raw(), (0,), (1,), F, "a refused call writes nothing")


# ================================================================================================ rotary embedding
def rotary(ctx, x, cos, sin, ids, mode, rot, interleaved, layout, leads=(0, 0, 0), what="", want=None):
    """rten_hip_rotary_embedding_f32 on guarded operands.  x is [B, S, H, D] in the rule's row order; layout "bshd" / "bhsd" says how it lies in memory."""
    b, s, h, d = x.shape
    mem = x if layout == "bshd" else np.ascontiguousarray(x.transpose(0, 2, 1, 3))
    st = (s * h * d, h * d, d) if layout == "bshd" else (h * s * d, d, s * d)
    xg, cg, sg = K.Guarded(ctx, mem, lead=leads[0]), K.Guarded(ctx, cos, lead=leads[1]), K.Guarded(ctx, sin, lead=leads[1])
    yg = K.Guarded(ctx, mem.nbytes, lead=leads[2])
    ig = K.Guarded(ctx, np.asarray(ids, np.int32)) if ids is not None else None
    half = rot // 2
    if mode == 0:
        cst = (0 if cos.shape[0] == 1 else cos.shape[1] * half, 0 if cos.shape[1] == 1 else half)
        sst = (0 if sin.shape[0] == 1 else sin.shape[1] * half, 0 if sin.shape[1] == 1 else half)
        max_pos = 0
    else:
        cst = sst = (0, 0)
        max_pos = cos.shape[0]
    ctx.call("rten_hip_rotary_embedding_f32", b, s, h, d, rot, 1 if interleaved else 0, xg.vp, *st, cg.vp, *cst, sg.vp, *sst, ig.vp if ig else None, mode, max_pos,
             yg.vp, *st)
    what = f"rotary {what} {x.shape} {layout} rot {rot} interleaved {interleaved} mode {mode} leads {leads}"
    got = yg.check(yg.raw(), mem.shape, K.dense(mem.shape), F, what)
    xg.check(xg.raw(), mem.shape, K.dense(mem.shape), F, what + " (the input)")
    if want is None:
        pos = None if mode == 0 else (np.asarray(ids) if mode == 1 else np.asarray(ids).reshape(-1)[0] + np.arange(s)[None, :].repeat(b, 0))
        if pos is not None:
            pos = R.clamp_ids(pos, max_pos)
        want4 = R.rotary_embedding(x.transpose(0, 2, 1, 3), cos, sin, pos, interleaved, 0, rot).transpose(0, 2, 1, 3)
        want = want4 if layout == "bshd" else want4.transpose(0, 2, 1, 3)
    same_bits(got, np.ascontiguousarray(want), what)
    return got


@pytest.mark.parametrize("d", [2, 4, 6, 64, 66, 128])
@pytest.mark.parametrize("interleaved", [False, True])
def test_rotary_every_shape_cache_and_position_form(ctx, d, interleaved):
    n = 0
    for b in (1, 2):
        for s in (1, 3):
            for h in (1, 3):
                for rot in sorted({0, 2, d - 2, d}):
                    n += 1
                    x = noise(n, b, s, h, d)
                    half = rot // 2
                    layout = ("bshd", "bhsd")[n % 2]
                    if rot == 0:  # nothing is rotated: the row is copied
                        rotary(ctx, x, np.zeros((1, 1, 0), F), np.zeros((1, 1, 0), F), None, 0, 0, interleaved, layout, want=x if layout == "bshd" else x.transpose(0, 2, 1, 3))
                        continue
                    cb, cs = (1, b)[n % 2], (1, s)[(n // 2) % 2]
                    rotary(ctx, x, noise(n + 1, cb, cs, half), noise(n + 2, (1, b)[(n // 4) % 2], cs, half), None, 0, rot, interleaved, layout, what="caches by (b, s)")
                    cos, sin = noise(n + 3, 7, half), noise(n + 4, 7, half)
                    ids = np.random.default_rng(n).integers(-7, 7, (b, s))
                    rotary(ctx, x, cos, sin, ids, 1, rot, interleaved, ("bhsd", "bshd")[n % 2], leads=(0, 0, 0) if n % 3 else (1, 2, 3), what="ids")
                    rotary(ctx, x, cos, sin, [n % 4], 2, rot, interleaved, layout, what="offset")
    x = noise(d, 2, 3, 2, d)
    cos, sin = noise(5, 4, d // 2), noise(6, 4, d // 2)
    rotary(ctx, x, cos, sin, [[0, 1, 9], [-9, 3, 2]], 1, d, interleaved, "bshd", what="ids past the cache are clamped")
    rotary(ctx, x, cos, sin, [2], 2, d, interleaved, "bhsd", what="an offset that runs past the cache is clamped")


@pytest.mark.parametrize("d", [6, 64])
def test_rotary_reads_a_q_block_of_a_fused_projection_in_place(ctx, d):
    """[B, S, 3 * H * D]: q, k and v blocks side by side; q and k are rotated from where they lie into dense outputs, v's block and the gaps stay untouched."""
    b, s, h = 2, 3, 2
    qkv = noise(d, b, s, 3 * h * d)
    cos, sin = noise(1, 8, d // 2), noise(2, 8, d // 2)
    g = K.Guarded(ctx, qkv)
    cg, sg, og = K.Guarded(ctx, cos), K.Guarded(ctx, sin), K.Guarded(ctx, np.array([3], np.int32))
    for block in (0, 1):
        yg = K.Guarded(ctx, b * s * h * d * 4)
        ctx.call("rten_hip_rotary_embedding_f32", b, s, h, d, d, 0, C.c_void_p(g.ptr + block * h * d * 4), s * 3 * h * d, 3 * h * d, d, cg.vp, 0, 0, sg.vp, 0, 0,
                 og.vp, 2, 8, yg.vp, s * h * d, h * d, d)
        got = yg.check(yg.raw(), (b, s, h * d), K.dense((b, s, h * d)), F, f"q/k block {block}")
        x = qkv[:, :, block * h * d:(block + 1) * h * d]
        same_bits(got, R.rotary_embedding_microsoft(x, np.array([3]), cos, sin, False, h, 0), f"block {block} of a fused projection")
    g.check(g.raw(), qkv.shape, K.dense(qkv.shape), F, "the projection is only read")
    # ... and written in place of the k block of another such buffer, on and one element off a 16-byte boundary: the q and v blocks and the guards keep their fill
    for lead in (0, 1):
        out = K.Guarded(ctx, qkv.nbytes, lead=lead)
        ctx.call("rten_hip_rotary_embedding_f32", b, s, h, d, d, 1, C.c_void_p(g.ptr + h * d * 4), s * 3 * h * d, 3 * h * d, d, cg.vp, 0, 0, sg.vp, 0, 0,
                 og.vp, 2, 8, C.c_void_p(out.ptr + h * d * 4), s * 3 * h * d, 3 * h * d, d)
        raw = out.raw()
        written = K.strided_mask(out.total, out.region + h * d * 4, 4, (b, s, h * d), (s * 3 * h * d, 3 * h * d, 1))
        K.assert_confined(raw, written, out.fill, "k block written in place of a strided destination", out.region + h * d * 4, 4, (s * 3 * h * d, 3 * h * d, 1), ("batch", "seq", "column"))
        got = np.lib.stride_tricks.as_strided(raw[out.region + h * d * 4:].view(F), (b, s, h * d), (s * 3 * h * d * 4, 3 * h * d * 4, 4))
        same_bits(np.ascontiguousarray(got), R.rotary_embedding_microsoft(qkv[:, :, h * d:2 * h * d], np.array([3]), cos, sin, True, h, 0), f"strided destination, interleaved, lead {lead}")


# ================================================================================================ the Python operators
def test_operators_defaults_axes_and_outputs(ctx):
    from rten_amd import einsum as E
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor as DT
    up = lambda a: DT.from_numpy(ctx, a)
    x = noise(1, 2, 3, 4, 10)
    g2 = noise(2, 4, 10)
    for cls in (ops.RMSNormalization, ops.SimplifiedLayerNormalization):
        same_bits(cls(axis=-2).run(ctx, [up(x), up(g2)])[0].numpy(), R.rms_normalization(x, g2, -2), "axis spanning two trailing dims")
        same_bits(cls().run(ctx, [up(x), up(g2[0])])[0].numpy(), R.rms_normalization(x, g2[0]), "defaults")
        same_bits(cls(epsilon=1e-3).run(ctx, [up(x), np.array([0.5], F)])[0].numpy(), R.rms_normalization(x, np.array([0.5], F), -1, 1e-3), "one-element scale")
        xt = E.View(up(x), [2, 4, 3, 10], [120, 10, 40, 1])
        same_bits(cls().run(ctx, [xt, up(g2[0])])[0].numpy(), R.rms_normalization(x.transpose(0, 2, 1, 3), g2[0]), "a strided input is re-laid")
    xs, skip, gamma, beta, bias = noise(3, 2, 3, 10), noise(4, 1, 3, 10), noise(5, 10), noise(6, 10), noise(7, 10)
    for rms in (False, True):
        op = ops.SkipSimplifiedLayerNormalization(1e-6) if rms else ops.SkipLayerNormalization(1e-6)
        ins = [up(xs), up(skip), up(gamma)] + ([up(bias)] if rms else [up(beta), up(bias)])
        want_y, want_t = R.skip_norm(xs, skip, gamma, None if rms else beta, bias, 1e-6, rms)
        out = op.run(ctx, ins)
        assert len(out) == 1
        same_bits(out[0].numpy(), want_y, f"skip rms {rms}")
        out = op.run(ctx, ins, outputs=[True, False, False, True])
        assert len(out) == 4 and out[1] is None and out[2] is None
        same_bits(out[0].numpy(), want_y, f"skip rms {rms} with the sum")
        same_bits(out[3].numpy(), want_t, f"skip rms {rms}: the sum")
        with pytest.raises(ops.OpError):
            op.run(ctx, ins, outputs=[True, True, False, False])
        one = np.array([1.5], F)  # a one-element gamma is the scalar form: other bits than a vector of equal values
        got = op.run(ctx, [up(xs), up(skip), up(one)], outputs=[True, False, False, True])
        want_y, want_t = R.skip_norm(xs, skip, one, None, None, 1e-6, rms)
        same_bits(got[0].numpy(), want_y, f"skip rms {rms}, one-element gamma")
        same_bits(got[3].numpy(), want_t, f"skip rms {rms}, one-element gamma: the sum")


def test_rotary_operators_positions_on_host_and_device(ctx):
    from rten_amd import einsum as E
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor as DT
    up = lambda a: DT.from_numpy(ctx, a)
    b, s, h, d = 2, 3, 2, 8
    x3, x4 = noise(1, b, s, h * d), noise(2, b, h, s, d)
    cos, sin = noise(3, 6, d // 2), noise(4, 6, d // 2)
    ids = np.array([[0, 5, 2], [1, 1, 4]], np.int32)
    for x, heads in ((x3, h), (x4, 0)):
        op = ops.RotaryEmbedding(num_heads=heads)
        same_bits(op.run(ctx, [up(x), up(cos), up(sin), up(ids)])[0].numpy(), R.rotary_embedding(x, cos, sin, ids, False, heads), "device ids")
        same_bits(op.run(ctx, [up(x), up(cos), up(sin), ids.astype(np.int64)])[0].numpy(), R.rotary_embedding(x, cos, sin, ids, False, heads), "host ids")
        c3, s3 = noise(5, 1, s, d // 2), noise(6, b, 1, d // 2)
        same_bits(ops.RotaryEmbedding(True, heads).run(ctx, [up(x), up(c3), up(s3)])[0].numpy(), R.rotary_embedding(x, c3, s3, None, True, heads), "no ids")
        ms = ops.RotaryEmbeddingMicrosoft(num_heads=heads or None)
        for k in (np.array(2, np.int32), np.array([3], np.int32)):
            want = R.rotary_embedding_microsoft(x, k, cos, sin, False, heads)
            same_bits(ms.run(ctx, [up(x), up(k), up(cos), up(sin)])[0].numpy(), want, "device offset")
            same_bits(ms.run(ctx, [up(x), k, up(cos), up(sin)])[0].numpy(), want, "host offset")
        same_bits(ms.run(ctx, [up(x), up(ids), up(cos), up(sin)])[0].numpy(), R.rotary_embedding_microsoft(x, ids, cos, sin, False, heads), "contrib ids")
    # one id past the cache: clamped on the device, refused on the host with Gather's message
    far = np.array([[0, 6, 2], [1, 1, -7]], np.int32)
    got = ops.RotaryEmbedding(num_heads=h).run(ctx, [up(x3), up(cos), up(sin), up(far)])[0].numpy()
    same_bits(got, R.rotary_embedding(x3, cos, sin, R.clamp_ids(far, 6), False, h), "clamped on the device")
    for bad in (far, ):
        with pytest.raises(ops.OpError) as e:
            ops.RotaryEmbedding(num_heads=h).run(ctx, [up(x3), up(cos), up(sin), bad])
        assert e.value == ops.InvalidValue("Entry in `indices` is out of range")
    with pytest.raises(ops.OpError) as e:
        ops.RotaryEmbeddingMicrosoft(num_heads=h).run(ctx, [up(x3), np.array([4], np.int32), up(cos), up(sin)])  # 4 + 2 is past the cache
    assert e.value == ops.InvalidValue("Entry in `indices` is out of range")
    got = ops.RotaryEmbeddingMicrosoft(num_heads=h).run(ctx, [up(x3), up(np.array([4], np.int32)), up(cos), up(sin)])[0].numpy()
    same_bits(got, R.rotary_embedding(x3, cos, sin, R.clamp_ids(4 + np.arange(3)[None, :].repeat(2, 0), 6), False, h), "offset clamped on the device")
    # a q block of a fused projection as a view: read in place
    qkv = up(noise(9, b, s, 3 * h * d))
    q = E.View(qkv, [b, s, h * d], [s * 3 * h * d, 3 * h * d, 1])
    want = R.rotary_embedding_microsoft(qkv.numpy()[:, :, :h * d], np.array(1), cos, sin, False, h)
    same_bits(ops.RotaryEmbeddingMicrosoft(num_heads=h).run(ctx, [q, np.array(1, np.int32), up(cos), up(sin)])[0].numpy(), want, "q block view")


# ================================================================================================ graphs
from tests.test_gpu_sample import run_cli_graph  # noqa: E402

CLI_MODES = [(), ("--no-fuse",), ("--graph",)]
B, S, H, D, MAXP = 2, 3, 2, 8, 16


def form_case(form):
    """(feeds, sizes, {output: expected}) of one norm_rotary_graph form at batch 2."""
    from rten_amd import onnx_writer as ow
    data, w = ow.norm_rotary_graph(form, seq=S, heads=H, head_size=D, max_pos=MAXP)
    x, skip = noise(1, B, S, H * D), noise(2, B, S, H * D)
    ids = np.array([[0, 7, 15], [3, 3, 1]], np.int32)
    feeds, want = {"x": x}, {}
    if form in ("rms", "simplified"):
        want["y"] = R.rms_normalization(x, w["gamma"], -1, 1e-6)
    elif form == "rms_two_axes":
        want["y"] = R.rms_normalization(x, w["gamma2"], -2)
    elif form == "rms_one_element_scale":
        want["y"] = R.rms_normalization(x, w["one"])
    elif form in ("skip_layer", "skip_layer_plain"):
        feeds["skip"] = skip
        y, t = R.skip_norm(x, skip, w["gamma"], w.get("beta"), w.get("bias"), 1e-5, False)
        want["y"] = y
        if form == "skip_layer":
            want["sum"] = t
    elif form in ("skip_simplified", "skip_simplified_batch_skip"):
        feeds["skip"] = skip if form == "skip_simplified" else skip[:1]
        want["y"], want["sum"] = R.skip_norm(x, feeds["skip"], w["gamma"], None, w["bias"], 1e-6, True)
    elif form in ("add_rms", "add_simplified_sole"):
        feeds["skip"] = skip
        t = (x + skip).astype(F)
        want["y"] = R.rms_normalization(t, w["gamma"], -1, 1e-6 if form == "add_rms" else None)
        if form == "add_rms":
            want["sum"] = t
    elif form == "rotary":
        want["y"] = R.rotary_embedding(x, w["cos3"], w["sin3"], None, False, H)
    elif form == "rotary_ids_4d":
        feeds = {"x": noise(3, B, H, S, D), "position_ids": ids}
        want["y"] = R.rotary_embedding(feeds["x"], w["cos"], w["sin"], ids)
    elif form == "rotary_interleaved_partial":
        feeds["position_ids"] = ids
        want["y"] = R.rotary_embedding(x, w["cos_part"], w["sin_part"], ids, True, H, D - 2)
    elif form == "ms_rotary_offset":
        feeds["offset"] = np.array([5], np.int32)
        want["y"] = R.rotary_embedding_microsoft(x, feeds["offset"], w["cos"], w["sin"], False, H)
    else:
        feeds["position_ids"] = ids
        want["y"] = R.rotary_embedding_microsoft(x, ids, w["cos"], w["sin"], False, None)
    return data, feeds, want


def _forms():
    from rten_amd import onnx_writer as ow
    return ow.NORM_ROTARY_FORMS


@pytest.mark.parametrize("form", _forms())
def test_every_operator_form_runs_eager_unfused_and_captured(ctx, tmp_path, form):
    data, feeds, want = form_case(form)
    for extra in CLI_MODES:
        got, log = run_cli_graph(tmp_path, data, feeds, list(want), {"batch": B}, extra)
        for name, w in want.items():
            same_bits(got[name].reshape(w.shape), w, f"{form} {extra} output {name}")
        if extra == ("--graph",):
            assert "Captured" in log, log[-1500:]
        if form.startswith("add_"):
            assert ("Add+" in log) == (extra != ("--no-fuse",)), log[-1500:]


BLOCK = dict(hidden=64, heads=4, kv_heads=2, head_size=16)


def block_case(batch=2, seq=2, past=3, offset=3, seed=7):
    """decoder_block_graph's feeds and the composition of decoder_rules with the oracle (matmul_f32, softmax) that its outputs must equal bit for bit."""
    from oracle import ref
    from rten_amd import onnx_writer as ow
    data, w = ow.decoder_block_graph(**BLOCK)
    heads, kv, d, hidden = BLOCK["heads"], BLOCK["kv_heads"], BLOCK["head_size"], BLOCK["hidden"]
    feeds = {"hidden_in": noise(seed, batch, seq, hidden), "residual_in": noise(seed + 1, batch, seq, hidden), "past_k": noise(seed + 2, batch, kv, past, d),
             "past_v": noise(seed + 3, batch, kv, past, d), "offset": np.array([offset], np.int32)}
    n1, res1 = R.skip_norm(feeds["hidden_in"], feeds["residual_in"], w["ln1_g"], None, None, 1e-6, True)
    q, k, v = (ref.matmul_f32(n1, w[nm]) for nm in ("wq", "wk", "wv"))
    q = R.rotary_embedding_microsoft(q, feeds["offset"], w["cos"], w["sin"], False, heads)
    k = R.rotary_embedding_microsoft(k, feeds["offset"], w["cos"], w["sin"], False, kv)
    split = lambda t, n: np.ascontiguousarray(t.reshape(batch, seq, n, d).transpose(0, 2, 1, 3))
    present_k = np.concatenate([feeds["past_k"], split(k, kv)], axis=2)
    present_v = np.concatenate([feeds["past_v"], split(v, kv)], axis=2)
    k_all, v_all = np.repeat(present_k, heads // kv, axis=1), np.repeat(present_v, heads // kv, axis=1)
    scores = ref.matmul_f32(split(q, heads), np.ascontiguousarray(k_all.transpose(0, 1, 3, 2)))
    probs = ref.softmax((scores * F(1.0 / np.sqrt(d))).astype(F))
    ctx4 = ref.matmul_f32(probs, np.ascontiguousarray(v_all))
    attn = ref.matmul_f32(np.ascontiguousarray(ctx4.transpose(0, 2, 1, 3)).reshape(batch, seq, hidden), w["wo"])
    n2, res2 = R.skip_norm(attn, res1, w["ln2_g"], None, None, 1e-6, True)
    gated = (R.silu(ref.matmul_f32(n2, w["w_gate"])) * ref.matmul_f32(n2, w["w_up"])).astype(F)
    want = {"mlp_out": ref.matmul_f32(gated, w["w_down"]), "residual_out": res2, "present_k": present_k, "present_v": present_v}
    return data, feeds, want


_BLOCK = {}


def shared_block_case():
    if not _BLOCK:
        _BLOCK["case"] = block_case()
    return _BLOCK["case"]


@pytest.mark.parametrize("extra", CLI_MODES + [("-t",)], ids=["fused", "unfused", "captured", "node by node"])
def test_decoder_block_graph_through_the_cli(ctx, tmp_path, extra):
    data, feeds, want = shared_block_case()
    got, log = run_cli_graph(tmp_path, data, feeds, list(want), {"batch": 2, "seq": 2, "past": 3}, extra)
    for name, w in want.items():
        same_bits(got[name].reshape(w.shape), w, f"decoder block {extra} output {name}")
    if extra == ("--graph",):
        assert "Captured" in log, log[-1500:]
    if extra == ("-t",):
        assert "SkipSimplifiedLayerNormalization" in log and "com.microsoft.RotaryEmbedding" in log, log[-3000:]


def test_decoder_block_through_the_c_abi_model_eager_and_captured(ctx):
    from rten_amd import lib as L
    from rten_amd.tensor import DeviceTensor
    # (the C-ABI model gives every input the same dim 0 -- the batch its chains split -- and `offset` is [1]: batch 1 here, batch 2 through the CLI above)
    data, feeds, want = block_case(batch=1, seq=2, past=3, offset=3, seed=9)

    def outputs(m):
        return {name: DeviceTensor(ctx, m.output(i)[1], F, ptr=m.output(i)[0], keepalive=m).numpy() for i, name in enumerate(m.outputs)}

    for captured in (False, True):
        m = L.Model(ctx, data)
        try:
            for name in m.inputs:
                a = feeds[name]
                DeviceTensor(ctx, a.shape, a.dtype, ptr=m.bind_input(name, a.shape), keepalive=m).upload(a)
            ctx.sync()
            if captured:
                m.prepare()
                m.run()
                m.sync()
            else:
                m.run_eager()
                ctx.sync()
            got = outputs(m)
            for name, w in want.items():
                same_bits(got[name].reshape(w.shape), w, f"decoder block, C-ABI model, captured {captured}, output {name}")
        finally:
            m.close()
    # one decode step after the prefill above: one new position, the caches one longer -- the shapes decode runs at (m == 1 products, one-row norms)
    data, feeds, want = block_case(batch=1, seq=1, past=5, offset=5, seed=11)
    m = L.Model(ctx, data)
    try:
        for name in m.inputs:
            a = feeds[name]
            DeviceTensor(ctx, a.shape, a.dtype, ptr=m.bind_input(name, a.shape), keepalive=m).upload(a)
        ctx.sync()
        m.prepare()
        m.run()
        m.sync()
        got = outputs(m)
        for name, w in want.items():
            same_bits(got[name].reshape(w.shape), w, f"decode step, output {name}")
    finally:
        m.close()


def test_loader_refusals_name_the_node(ctx, tmp_path):
    from rten_amd import onnx_writer as ow
    from tests.test_graph_executor import run_cli
    for form, words in (("stash_type_0", ("RMSNormalization norm", "stash_type")), ("skip_mean_read", ("SkipLayerNormalization skip_norm", "output 1")),
                        ("rms_int_scale", ("RMSNormalization norm", "float32 only"))):
        p = tmp_path / (form + ".onnx")
        p.write_bytes(ow.norm_rotary_graph(form)[0])
        r = run_cli("-s", "batch=1", str(p))
        assert r.returncode == 1 and all(wd in r.stderr for wd in words), r.stderr
