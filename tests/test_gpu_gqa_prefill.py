"""The fused prefill kernel of GroupQueryAttention (rten_amd/csrc/gqa_prefill.hip, rten_hip_set_gqa_path 4): the output and both presents bit for bit
against tests/gqa_rules.py at the strip (64 rows), key-tile (64 keys) and PV depth-block (256 keys) boundaries, windows whose low bound skips tiles and a
whole depth block, operands that a skipped tile must not hide, its refusals, one capture replayed at three lengths, mode 0 and one float64 check."""
import ctypes as C

import numpy as np
import pytest

from tests import attention_rules as A
from tests import gqa_rules as G
from tests.reduce_rules import same_bits
from tests.test_gpu_gqa import gqa, noise, tables

F, I = np.float32, np.int32
pytestmark = pytest.mark.gpu

AUTO, COMPOSED, PREFILL = 0, 1, 4  # rten_hip_set_gqa_path
ALIGNED = (0, 4, 8)  # leads that keep the output and both presents on 16 bytes: the 16-byte loads and stores (gqa()'s default leads take the 4-byte forms)


def operands(seed, batch, h, kv, seq, past, d, rand=noise):
    q, k, v = rand(seed, batch, seq, h * d), rand(seed + 1, batch, seq, kv * d), rand(seed + 2, batch, seq, kv * d)
    return (q, k, v, rand(seed + 3, batch, kv, past, d), rand(seed + 4, batch, kv, past, d)) if past else (q, k, v, None, None)


# S: a partial strip, one strip, a strip boundary; T = past + S on 63 / 64 / 65 (key tile), 255 / 256 / 257 and 513 (PV fold: two and three depth blocks)
SHAPES = [  # S, past, d, h, kv
    (2, 61, 64, 4, 4), (63, 1, 128, 8, 2), (64, 1, 64, 16, 1), (65, 0, 128, 4, 4), (130, 0, 64, 8, 2), (2, 253, 128, 16, 1), (64, 192, 64, 8, 2),
    (65, 192, 128, 8, 2), (63, 450, 64, 4, 4), (130, 383, 128, 8, 2),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "s%d-past%d-d%d-h%d-kv%d" % s)
def test_prefill_kernel_at_its_boundaries(ctx, shape):
    seq, past, d, h, kv = shape
    t = past + seq
    batch = 1 if past else 2  # (the rule, like the reference, takes a chunk on a past at batch 1 only)
    gqa(ctx, *operands(t + d, batch, h, kv, seq, past, d), [t - 1] * batch, t, h=h, kv=kv, path=PREFILL, leads=ALIGNED if seq % 2 else (1, 2, 3))


# S = 130 on a past of 190: rows 190 .. 319.  Window 1: the low bound inside a tile, one key a row; 64: strip 1's on the tile boundary 256, so its first
# depth block is skipped whole and the second is the one stored; 65 and 200: inside a tile, strip 0 of 200 unbounded below
WINDOWS = {
    1: lambda s, t, h, d: dict(bias=noise(41, 1, 1, s, t), **dict(zip(("cos", "sin"), tables(42, t + 5, d // 2)))),
    64: lambda s, t, h, d: dict(bias=noise(43, 1, h, s + 1, t + 2)),
    65: lambda s, t, h, d: dict(interleaved=True, **dict(zip(("cos", "sin"), tables(44, t + 5, d // 4)))),
    200: lambda s, t, h, d: dict(packed=True, **dict(zip(("cos", "sin"), tables(45, t + 5, d // 2)))),
}


@pytest.mark.parametrize("window", list(WINDOWS))
def test_windows_bias_rotary_and_packed_qkv(ctx, window):
    seq, past, h, kv, d = 130, 190, 8, 2, 64 if window in (1, 65) else 128
    t = past + seq
    kw = WINDOWS[window](seq, t, h, d)
    q, k, v, pk, pv = operands(window, 1, h, kv, seq, past, d)
    if kw.get("packed"):
        q, k, v = np.concatenate([q, k, v], axis=2), None, None
    gqa(ctx, q, k, v, pk, pv, [t - 1], t, h=h, kv=kv, window=window, path=PREFILL, leads=ALIGNED if window != 65 else (3, 1, 2), **kw)


def test_right_padded_batch_has_the_composed_path_s_bits(ctx):
    """A first prompt of 65 rows into caches of T = 165 rows, seqlens_k [T - 1, T - 70]: the rule's products stop at each item's kv_len, both paths here walk
    all T columns, the zero rows from 65 on with probability +0.  (gqa() holds both to the rule's bits, which is more than `==`.)"""
    seq, past, h, kv, d = 65, 100, 8, 2, 128
    t = past + seq
    ops = operands(5, 2, h, kv, seq, past, d)
    fused, composed = (gqa(ctx, *ops, [t - 1, t - 70], seq, h=h, kv=kv, path=path, leads=ALIGNED) for path in (PREFILL, COMPOSED))
    for a, b, name in zip(fused, composed, ("output", "present_key", "present_value")):
        same_bits(a, b, f"mode 4 against mode 1 ({name})")
        assert np.array_equal(a, b)


def test_skipped_tiles_do_not_hide_their_operands(ctx):
    """A first prompt of 130 rows: sweep C would skip key tile 1 (keys 64 .. 127) for strip 0 (rows 0 .. 63), and a window of 64 on a past of 190 skips tile 0
    for every strip."""
    seq, h, kv, d = 130, 8, 2, 64
    q, k, v, _, _ = operands(6, 1, h, kv, seq, 0, d)
    run = lambda k_, v_: gqa(ctx, q, k_, v_, None, None, [seq - 1], seq, h=h, kv=kv, path=PREFILL, leads=ALIGNED)[0]
    clean = run(k, v)
    bad_v = v.copy()
    bad_v[0, 100] = np.nan
    assert np.isnan(run(k, bad_v)).all()  # 0 * NaN in every row, as the rule says (gqa() compares the bits)
    bad_k = k.copy()
    bad_k[0, 100] = np.nan
    got = run(bad_k, v)
    same_bits(got[:, :100], clean[:, :100], "rows that end before the NaN key")
    assert not got[:, 100:].any()
    q, k, v, pk, pv = operands(7, 1, h, kv, seq, 190, d)
    pv[0, :, 10] = np.inf  # outside [start, lim) of every row, inside kv_len
    assert np.isnan(gqa(ctx, q, k, v, pk, pv, [319], 320, h=h, kv=kv, window=64, path=PREFILL, leads=ALIGNED)[0]).all()


@pytest.mark.parametrize("seq,d", [(2, 80), (1, 64)], ids=["head-size-80", "one-row-gemv-order"])
def test_mode_4_refuses_what_the_kernel_does_not_cover(ctx, seq, d):
    from rten_amd import lib as L
    ops = operands(8, 1, 4, 2, seq, 5, d)
    with pytest.raises(L.HipError):
        gqa(ctx, *ops, [4 + seq], 5 + seq, h=4, kv=2, path=PREFILL)
    gqa(ctx, *ops, [4 + seq], 5 + seq, h=4, kv=2)  # the automatic path still works


def test_one_captured_call_follows_new_device_lengths(ctx):
    """S = 70 on a 256-row cache: one captured call replayed with seqlens_k of 255, 200 and 100, each several times."""
    from rten_amd.tensor import DeviceTensor
    dev = lambda a: DeviceTensor.from_numpy(ctx, np.ascontiguousarray(a))
    h, kv, d, seq, past = 8, 2, 64, 70, 186
    t = past + seq
    q, k, v, pk, pv = operands(9, 1, h, kv, seq, past, d)
    cos, sin = tables(10, t, d // 2)
    tq, tk, tv, tpk, tpv, tcos, tsin = (dev(a) for a in (q, k, v, pk, pv, cos, sin))
    seqlens, total = dev(np.array([t - 1], I)), dev(np.array([t], I))
    out, ok, ov = (DeviceTensor(ctx, s, F) for s in ((1, seq, h * d), (1, kv, t, d), (1, kv, t, d)))
    dims = (C.c_int32 * 10)(1, seq, h, kv, d, past, d, 0, t, 0)
    st = (C.c_int64 * 12)(seq * h * d, h * d, d, seq * kv * d, kv * d, d, seq * kv * d, kv * d, d, 0, 0, 0)

    def launch():
        ctx.call("rten_hip_gqa_f32", dims, st, 0.125, tq.vp, tk.vp, tv.vp, tpk.vp, tpv.vp, seqlens.vp, total.vp, tcos.vp, tsin.vp, None, None, out.vp, ok.vp, ov.vp)

    ctx.call("rten_hip_set_gqa_path", PREFILL)
    graph = None
    try:
        launch()  # warm-up: the rotated Q's scratch is sized outside the capture
        ctx.sync()
        ctx.graph_begin()
        launch()
        graph = ctx.graph_end()
        for n in (255, 200, 100):
            seqlens.upload(np.array([n], I))
            for _ in range(2):
                ctx.graph_launch(graph)
            ctx.sync()
            want = G.group_query_attention(q, k, v, pk, pv, [n], t, cos, sin, num_heads=h, kv_num_heads=kv, scale=0.125, do_rotary=True)
            for got, w, name in zip((out, ok, ov), want, ("output", "present_key", "present_value")):
                same_bits(got.numpy(), w, f"replay with seqlens_k {n} ({name})")
    finally:
        ctx.call("rten_hip_set_gqa_path", AUTO)
        if graph is not None:
            ctx.graph_destroy(graph)


def test_mode_0_gives_mode_4_bits_inside_the_rule(ctx):
    """A first prompt of 2048 rows at head size 64 on 1024 workgroups: the rule's smallest shape.  Device against device: the rule is held above."""
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    h, kv, d, seq = 32, 8, 64, 2048
    dev = [DeviceTensor.from_numpy(ctx, a) for a in operands(12, 1, h, kv, seq, 0, d)[:3]] + [None, None, np.array([seq - 1], I), np.array(seq, I)]
    got = []
    for path in (AUTO, PREFILL):
        ctx.call("rten_hip_set_gqa_path", path)
        try:
            got.append(ops.GroupQueryAttention(h, kv).run(ctx, dev, outputs=(0,))[0].numpy())
        finally:
            ctx.call("rten_hip_set_gqa_path", AUTO)
    same_bits(got[0], got[1], "mode 0 against mode 4")


def test_against_float64_attention(ctx):
    """A causal chunk on a past; uniform [0, 1) operands and the bound 1e-8 + 1e-5 |want| that tests/test_attention_ops.py holds the rule to."""
    b, h, kv, seq, past, d = 1, 8, 2, 65, 70, 128
    q, k, v, pk, pv = operands(11, b, h, kv, seq, past, d, rand=lambda seed, *shape: np.random.default_rng(seed).random(shape, dtype=F))
    t = past + seq
    out, present_k, present_v = gqa(ctx, q, k, v, pk, pv, [t - 1] * b, t, h=h, kv=kv, path=PREFILL, leads=ALIGNED)
    want = A.naive(q.reshape(b, seq, h, d).transpose(0, 2, 1, 3), present_k, present_v, None, past, None, True, float(F(1.0) / np.sqrt(F(d))))
    got = out.reshape(b, seq, h, d).transpose(0, 2, 1, 3)
    assert np.all(np.abs(got - want) <= 1e-8 + 1e-5 * np.abs(want)), np.abs(got - want).max()
