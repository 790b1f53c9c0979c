"""com.microsoft.GroupQueryAttention with a KV cache on the device (rten_amd/csrc/gqa.hip): rten_hip_gqa_f32 bit for bit against tests/gqa_rules.py on guarded,
misaligned outputs -- the one-launch decode kernel at every length at which its orders change (the under-8 left-over keys, the 128-key column block edge, the
8-key depth block tail), windows, bias, rotary in both pairings with and without position_ids; the composed path for other head sizes, the gemv order switched
off and rows past the decode kernel's LDS bound; prefill (first prompt, appended chunks across the 256 depth block and the 512-key reach, packed QKV read in
place); both present caches with zero rows and dropped rows; NaN and out-of-range device values confined; then the Python operator and one captured launch
replayed with new device lengths; and onnx_writer.decoder_block_gqa_graph in its three forms through the CLI (fused, unfused, captured, node by node) and the
C-ABI model (eager, captured, one captured plan replayed at three lengths)."""
import ctypes as C

import numpy as np
import pytest

from tests import confine as K
from tests import gqa_rules as G
from tests.reduce_rules import same_bits

F, I = np.float32, np.int32
pytestmark = pytest.mark.gpu

AUTO, COMPOSED, DECODE = 0, 1, 2  # rten_hip_set_gqa_path


def noise(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


def tables(seed, max_pos, half):
    ang = np.random.default_rng(seed).uniform(0, 6.28, (max_pos, half))
    return np.cos(ang).astype(F), np.sin(ang).astype(F)


def gqa(ctx, q, k, v, pk, pv, seqlens, total, *, h, kv, scale=None, cos=None, sin=None, pos=None, bias=None, interleaved=False, window=None, path=AUTO,
        packed=False, leads=(1, 2, 3), want_seqlens=None, what=""):
    """rten_hip_gqa_f32 on guarded operands -> (out, present_k, present_v), each confined and bit-equal to the rule.  packed: q is [B, S, (H + 2 KV) * D] and
    k, v are read out of it in place.  want_seqlens: the values the rule is asked (device values that the kernels clamp)."""
    batch, seq = q.shape[:2]
    d = q.shape[2] // (h + 2 * kv if packed else h)
    past = 0 if pk is None else pk.shape[2]
    t = past + seq
    qg = K.Guarded(ctx, q)
    if packed:
        row = (h + 2 * kv) * d
        ptrs = [qg.ptr, qg.ptr + 4 * h * d, qg.ptr + 4 * (h + kv) * d]
        strides = [seq * row, row, d] * 3
        keep = [qg]
    else:
        kg, vg = K.Guarded(ctx, k), K.Guarded(ctx, v)
        ptrs, keep = [qg.ptr, kg.ptr, vg.ptr], [qg, kg, vg]
        strides = [seq * h * d, h * d, d] + [seq * kv * d, kv * d, d] * 2
    pkg, pvg = (K.Guarded(ctx, pk), K.Guarded(ctx, pv)) if past else (None, None)
    sg, tg = K.Guarded(ctx, np.asarray(seqlens, I)), K.Guarded(ctx, np.asarray([total], I))
    cg, ng = (K.Guarded(ctx, cos), K.Guarded(ctx, sin)) if cos is not None else (None, None)
    pg = K.Guarded(ctx, np.asarray(pos, I)) if pos is not None else None
    bg, bst = None, [0, 0, 0]
    if bias is not None:
        bg = K.Guarded(ctx, bias)
        bb, bh, bs, bt = bias.shape
        bst = [0 if bb == 1 else bh * bs * bt, 0 if bh == 1 else bs * bt, bt]
    og = K.Guarded(ctx, batch * seq * h * d * 4, lead=leads[0])
    okg, ovg = K.Guarded(ctx, batch * kv * t * d * 4, lead=leads[1]), K.Guarded(ctx, batch * kv * t * d * 4, lead=leads[2])
    rot = 0 if cos is None else 2 * cos.shape[1]
    dims = (C.c_int32 * 10)(batch, seq, h, kv, d, past, rot, int(interleaved), 0 if cos is None else cos.shape[0], window or 0)
    st = (C.c_int64 * 12)(*strides, *bst)
    sc = float(F(1.0) / np.sqrt(F(d))) if scale is None else scale
    vp = lambda g: g.vp if g is not None else None
    ctx.call("rten_hip_set_gqa_path", path)
    try:
        ctx.call("rten_hip_gqa_f32", dims, st, sc, *(C.c_void_p(p) for p in ptrs), vp(pkg), vp(pvg), sg.vp, tg.vp, vp(cg), vp(ng), vp(pg), vp(bg), og.vp,
                 okg.vp, ovg.vp)
    finally:
        ctx.call("rten_hip_set_gqa_path", AUTO)
    what = f"gqa {what} B {batch} S {seq} H {h} KV {kv} D {d} P {past} seqlens {list(seqlens)} total {total} window {window} bias {bias is not None} " \
           f"rot {rot} interleaved {interleaved} pos {pos is not None} packed {packed} path {path}"
    out = og.check(og.raw(), (batch, seq, h * d), K.dense((batch, seq, h * d)), F, what + " (output)")
    shape = (batch, kv, t, d)
    got_k = okg.check(okg.raw(), shape, K.dense(shape), F, what + " (present_key)")
    got_v = ovg.check(ovg.raw(), shape, K.dense(shape), F, what + " (present_value)")
    want = G.group_query_attention(q, None if packed else k, None if packed else v, pk, pv, seqlens if want_seqlens is None else want_seqlens, total, cos, sin,
                                   pos, bias, num_heads=h, kv_num_heads=kv, scale=scale, do_rotary=cos is not None, rotary_interleaved=interleaved,
                                   local_window_size=window)
    same_bits(got_k, want[1], what + " (present_key)")
    same_bits(got_v, want[2], what + " (present_value)")
    same_bits(out, want[0], what + " (output)")
    del keep
    return out, got_k, got_v


def decode_operands(seed, batch, h, kv, d, past):
    return noise(seed, batch, 1, h * d), noise(seed + 1, batch, 1, kv * d), noise(seed + 2, batch, 1, kv * d), noise(seed + 3, batch, kv, past, d), \
        noise(seed + 4, batch, kv, past, d)


# the lengths at which the decode kernel's orders change, as pairs so that the two batch items differ (the shorter item is right-padded)
KV_PAIRS = [(1, 7), (8, 9), (127, 128), (129, 135), (257, 200)]


# ================================================================================================ the decode kernel
@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (8, 1)], ids=lambda p: "h%d-kv%d" % p)
@pytest.mark.parametrize("d", [64, 128])
def test_decode_kernel_every_length_window_and_bias(ctx, d, heads):
    h, kv = heads
    for a, b in KV_PAIRS:
        past = max(a, b) - 1
        ops = decode_operands(a + d, 2, h, kv, d, past)
        gqa(ctx, *ops, [a - 1, b - 1], past + 2, h=h, kv=kv, path=DECODE)
    a, b = 135, 129
    past = 134
    ops = decode_operands(7, 2, h, kv, d, past)
    bias = noise(9, 2, h, 1, past + 3)
    gqa(ctx, *ops, [a - 1, b - 1], 200, h=h, kv=kv, window=4, path=DECODE)
    gqa(ctx, *ops, [a - 1, b - 1], 200, h=h, kv=kv, window=200, bias=bias, scale=0.3, path=DECODE)
    gqa(ctx, *ops, [a - 1, b - 1], 200, h=h, kv=kv, window=130, bias=noise(10, 1, 1, 2, past + 1), path=DECODE)


@pytest.mark.parametrize("d", [64, 128])
def test_decode_kernel_with_rotary(ctx, d):
    h, kv, past = 8, 2, 40
    ops = decode_operands(d, 2, h, kv, d, past)
    for rot in (d, d // 2):
        cos, sin = tables(rot, 64, rot // 2)
        for interleaved in (False, True):
            gqa(ctx, *ops, [40, 22], 41, h=h, kv=kv, cos=cos, sin=sin, interleaved=interleaved, path=DECODE)
        gqa(ctx, *ops, [40, 22], 41, h=h, kv=kv, cos=cos, sin=sin, pos=[[63], [5]], path=DECODE)


def test_decode_kernel_is_the_automatic_choice_and_refuses_what_it_does_not_cover(ctx):
    from rten_amd import lib as L
    ops = decode_operands(3, 1, 4, 2, 64, 5)
    auto = gqa(ctx, *ops, [5], 6, h=4, kv=2)[0]
    same_bits(auto, gqa(ctx, *ops, [5], 6, h=4, kv=2, path=DECODE)[0], "automatic path")
    with pytest.raises(L.HipError):
        gqa(ctx, *decode_operands(3, 1, 4, 2, 80, 5), [5], 6, h=4, kv=2, path=DECODE)
    with pytest.raises(L.HipError):  # one row in the gemv order with a head size above 512 (a second depth block): refused, not approximated
        gqa(ctx, *decode_operands(3, 1, 1, 1, 528, 2), [2], 3, h=1, kv=1)


# ================================================================================================ fallback routing (one query row on the composed path)
@pytest.mark.parametrize("d", [8, 80])
def test_other_head_sizes_take_the_composed_path(ctx, d):
    for past in (5, 130):
        gqa(ctx, *decode_operands(d + past, 2, 4, 2, d, past), [past, past], past + 1, h=4, kv=2)
    # right-padded items: the left-over keys of a column block follow each item's own kv_len (1 | 7, 8 | 9, 127 | 128, 129 | 135, 257 | 200)
    for a, b in KV_PAIRS:
        past = max(a, b) - 1
        gqa(ctx, *decode_operands(a + d, 2, 4, 2, d, past), [a - 1, b - 1], past + 2, h=4, kv=2, what="right-padded")
    for a, b in KV_PAIRS[1:]:  # the same on the composed path at a head size the decode kernel covers
        past = max(a, b) - 1
        gqa(ctx, *decode_operands(a, 2, 8, 2, 64, past), [a - 1, b - 1], past + 2, h=8, kv=2, path=COMPOSED, what="right-padded, composed by choice")
    gqa(ctx, *decode_operands(d, 1, 4, 2, d, 9), [9], 10, h=4, kv=2, window=4, bias=noise(1, 1, 4, 1, 10))


def test_gemv_order_off_takes_the_blocked_order(ctx):
    from oracle import ref
    ctx.call("rten_hip_set_gemv_order", 0, 0)
    ref.set_gemv_enabled(False)
    try:
        for d in (64, 80):
            gqa(ctx, *decode_operands(d, 2, 8, 2, d, 135), [135, 135], 136, h=8, kv=2)
            gqa(ctx, *decode_operands(d, 2, 8, 2, d, 135), [135, 128], 200, h=8, kv=2, what="right-padded")
    finally:
        ctx.call("rten_hip_set_gemv_order", 1, 0)
        ref.set_gemv_enabled(True)


def test_rows_past_the_lds_bound_take_the_composed_path(ctx):
    """4 * (G * (P + 1 + D) + 8192) <= 160 KiB: G = 8, D = 64 admits P + 1 <= 4032 keys."""
    from rten_amd import lib as L
    h, kv, d = 8, 1, 64
    for past, covered in ((4031, True), (4032, False)):
        assert (4 * (8 * (past + 1 + d) + 8192) <= 160 * 1024) == covered
        ops = decode_operands(past, 1, h, kv, d, past)
        if covered:
            gqa(ctx, *ops, [past], past + 1, h=h, kv=kv, path=DECODE, what="at the bound")
        else:
            gqa(ctx, *ops, [past], past + 1, h=h, kv=kv, what="past the bound")
            gqa(ctx, *decode_operands(past, 2, h, kv, d, past), [past, past - 5], past + 9, h=h, kv=kv, what="past the bound, right-padded")
            with pytest.raises(L.HipError):
                gqa(ctx, *ops, [past], past + 1, h=h, kv=kv, path=DECODE)


# ================================================================================================ prefill
@pytest.mark.parametrize("seq", [3, 130])
def test_first_prompt(ctx, seq):
    h, kv, d = 4, 2, 64
    q, k, v = noise(seq, 2, seq, h * d), noise(seq + 1, 2, seq, kv * d), noise(seq + 2, 2, seq, kv * d)
    gqa(ctx, q, k, v, None, None, [seq - 1, seq - 1], seq, h=h, kv=kv)
    cos, sin = tables(1, seq + 3, 16)
    gqa(ctx, q[:1], k[:1], v[:1], None, None, [seq - 1], seq, h=h, kv=kv, cos=cos, sin=sin, window=2, what="rotary, window")


@pytest.mark.parametrize("past", [2, 255, 509])
def test_chunk_appended_to_a_full_cache(ctx, past):
    """S = 5 on P = 2 and 255 (PV crosses the 256 depth block), and P + S = 514, just past the fused attention kernel's 512-key reach."""
    h, kv, d, seq = 4, 2, 64, 5
    q, k, v = noise(past, 1, seq, h * d), noise(past + 1, 1, seq, kv * d), noise(past + 2, 1, seq, kv * d)
    pk, pv = noise(past + 3, 1, kv, past, d), noise(past + 4, 1, kv, past, d)
    gqa(ctx, q, k, v, pk, pv, [past + seq - 1], past + seq, h=h, kv=kv)
    if past == 2:
        gqa(ctx, q, k, v, pk, pv, [past + seq - 1], past + seq, h=h, kv=kv, bias=noise(5, 1, h, seq + 1, past + seq + 2), window=3, what="bias, window")


def test_long_prompt_runs_in_two_passes_over_the_query_rows(ctx):
    """H * S * (P + S) * 4 bytes = 70.6 MB of scores: above the 64 MiB a pass of the composed path may hold, so the rows run in two passes."""
    h, kv, d, seq = 4, 2, 64, 2100
    assert h * seq * seq * 4 > 64 << 20 > h * seq * seq * 2
    q, k, v = noise(1, 1, seq, h * d), noise(2, 1, seq, kv * d), noise(3, 1, seq, kv * d)
    gqa(ctx, q, k, v, None, None, [seq - 1], seq, h=h, kv=kv, window=700)


def test_packed_qkv_is_read_in_place(ctx):
    h, kv, d = 4, 2, 64
    for seq, past in ((3, 0), (1, 9)):
        packed = noise(seq, 2 if seq == 3 else 1, seq, (h + 2 * kv) * d)
        pk = pv = None
        if past:
            pk, pv = noise(1, 1, kv, past, d), noise(2, 1, kv, past, d)
        cos, sin = tables(2, 16, d // 2)
        gqa(ctx, packed, None, None, pk, pv, [past + seq - 1] * packed.shape[0], past + seq, h=h, kv=kv, packed=True, cos=cos, sin=sin)


# ================================================================================================ confinement
def test_nan_in_dropped_past_rows_and_beyond_the_causal_limit_is_confined(ctx):
    h, kv, d, past = 8, 2, 64, 20
    q, k, v, pk, pv = decode_operands(11, 2, h, kv, d, past)
    pk[1, :, 9:], pv[1, :, 9:] = np.nan, np.nan  # item 1 has past_len 9: these rows are dropped
    out = gqa(ctx, q, k, v, pk, pv, [20, 9], 30, h=h, kv=kv, path=DECODE)[0]
    assert np.isfinite(out).all()
    assert np.isfinite(gqa(ctx, q, k, v, pk, pv, [20, 9], 30, h=h, kv=kv, path=COMPOSED, leads=(3, 1, 2))[0]).all()
    # prefill: a NaN key row 2 is beyond the causal limit of queries 0 and 1
    seq = 4
    q, k, v = noise(1, 1, seq, h * d), noise(2, 1, seq, kv * d), noise(3, 1, seq, kv * d)
    clean = gqa(ctx, q, k, v, None, None, [seq - 1], seq, h=h, kv=kv)[0]
    k[0, 2] = np.nan
    out = gqa(ctx, q, k, v, None, None, [seq - 1], seq, h=h, kv=kv)[0]
    same_bits(out[:, :2], clean[:, :2], "queries that end before the NaN row")
    assert not out[:, 2:].any()  # a NaN score makes the row's sum NaN, and the softmax flushes the whole row to zero (attention.rs:549-551)
    # a window keeps a NaN key row out of a decode query as well
    q, k, v, pk, pv = decode_operands(12, 1, h, kv, d, past)
    pk[0, :, 3] = np.nan
    assert np.isfinite(gqa(ctx, q, k, v, pk, pv, [20], 21, h=h, kv=kv, window=5, path=DECODE)[0]).all()


@pytest.mark.parametrize("path", [DECODE, COMPOSED])
def test_out_of_range_device_lengths_write_only_inside_the_outputs(ctx, path):
    h, kv, d, past = 4, 2, 64, 12
    ops = decode_operands(13, 2, h, kv, d, past)
    # kv_len is clamped into [1, P + 1]: -5 behaves as 0, 1000 as P
    gqa(ctx, *ops, [-5, 1000], 50, h=h, kv=kv, path=path, want_seqlens=[0, past])
    gqa(ctx, *ops, [2 ** 31 - 1, -2 ** 31], 50, h=h, kv=kv, path=path, want_seqlens=[past, 0])


# ================================================================================================ the Python operator
def test_operator_host_values_raise_the_reference_s_value_errors(ctx):
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    dev = lambda a: DeviceTensor.from_numpy(ctx, np.ascontiguousarray(a))
    op = ops.GroupQueryAttention(2, 1)
    q, k, v = dev(np.zeros((1, 2, 16), F)), dev(np.zeros((1, 2, 8), F)), dev(np.zeros((1, 2, 8), F))
    for seqlens, total in (([0], 1), ([0], 2)):
        with pytest.raises(ops.OpError) as e:
            op.run(ctx, [q, k, v, None, None, np.array(seqlens, I), np.array(total, I)])
        assert e.value == ops.InvalidValue("seqlens_k entry is too small for the query sequence length")
    q1, k1, v1, past = dev(np.zeros((1, 1, 16), F)), dev(np.zeros((1, 1, 8), F)), dev(np.zeros((1, 1, 8), F)), dev(np.zeros((1, 1, 2, 8), F))
    with pytest.raises(ops.OpError) as e:
        op.run(ctx, [q1, k1, v1, past, past, np.array([9], I), np.array(10, I)])
    assert e.value == ops.InvalidValue("seqlens_k entry is out of range")
    with pytest.raises(ops.OpError) as e:
        op.run(ctx, [q1, k1, v1, past, past, np.array([2], I), np.array(0, I)])
    assert e.value == ops.InvalidValue("total_sequence_length must be positive")


def test_operator_matches_the_rule_with_host_and_device_lengths(ctx):
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    dev = lambda a: DeviceTensor.from_numpy(ctx, np.ascontiguousarray(a))
    h, kv, d, past = 8, 2, 64, 17
    q, k, v, pk, pv = decode_operands(21, 2, h, kv, d, past)
    cos, sin = tables(3, 32, d // 2)
    bias = noise(4, 1, h, 1, past + 1)
    seqlens, total = np.array([[17], [6]], I), np.array(18, I)  # [B, 1] is accepted
    want = G.group_query_attention(q, k, v, pk, pv, seqlens, total, cos, sin, None, bias, num_heads=h, kv_num_heads=kv, do_rotary=True, local_window_size=9)
    op = ops.GroupQueryAttention(h, kv, do_rotary=True, local_window_size=9)
    for lengths in ((seqlens, total), (dev(seqlens), dev(total))):
        outs = op.run(ctx, [dev(q), dev(k), dev(v), dev(pk), dev(pv), *lengths, dev(cos), dev(sin), None, dev(bias)])
        assert len(outs) == 3
        for got, w, name in zip(outs, want, ("output", "present_key", "present_value")):
            same_bits(got.numpy(), w, name)
    assert len(op.run(ctx, [dev(q), dev(k), dev(v), dev(pk), dev(pv), seqlens, total, dev(cos), dev(sin), None, dev(bias)], outputs=(0,))) == 1
    # packed QKV through the operator
    packed = noise(5, 1, 3, (h + 2 * kv) * d)
    want = G.group_query_attention(packed, None, None, None, None, [2], 3, num_heads=h, kv_num_heads=kv)
    outs = ops.GroupQueryAttention(h, kv).run(ctx, [dev(packed), None, None, None, None, np.array([2], I), np.array(3, I)])
    for got, w in zip(outs, want):
        same_bits(got.numpy(), w, "packed")


# ================================================================================================ capture
def test_one_captured_launch_follows_new_device_lengths(ctx):
    """past = 6, S = 1: a captured launch replayed with seqlens_k of 2, 3 and 4 written to the device input -- nothing is baked in at capture."""
    from rten_amd.tensor import DeviceTensor
    dev = lambda a: DeviceTensor.from_numpy(ctx, np.ascontiguousarray(a))
    h, kv, d, past = 8, 2, 64, 6
    q, k, v, pk, pv = decode_operands(31, 1, h, kv, d, past)
    cos, sin = tables(6, 16, d // 2)
    tq, tk, tv, tpk, tpv, tcos, tsin = (dev(a) for a in (q, k, v, pk, pv, cos, sin))
    seqlens, total = dev(np.array([6], I)), dev(np.array([7], I))
    out, ok, ov = (DeviceTensor(ctx, s, F) for s in ((1, 1, h * d), (1, kv, past + 1, d), (1, kv, past + 1, d)))
    dims = (C.c_int32 * 10)(1, 1, h, kv, d, past, d, 0, 16, 0)
    st = (C.c_int64 * 12)(h * d, h * d, d, kv * d, kv * d, d, kv * d, kv * d, d, 0, 0, 0)

    def launch():
        ctx.call("rten_hip_gqa_f32", dims, st, 0.125, tq.vp, tk.vp, tv.vp, tpk.vp, tpv.vp, seqlens.vp, total.vp, tcos.vp, tsin.vp, None, None, out.vp, ok.vp, ov.vp)

    launch()  # warm-up: scratch is sized outside the capture
    ctx.sync()
    ctx.graph_begin()
    launch()
    graph = ctx.graph_end()
    try:
        for n in (2, 3, 4):
            seqlens.upload(np.array([n], I))
            ctx.graph_launch(graph)
            ctx.sync()
            want = G.group_query_attention(q, k, v, pk, pv, [n], 7, cos, sin, num_heads=h, kv_num_heads=kv, scale=0.125, do_rotary=True)
            for got, w, name in zip((out, ok, ov), want, ("output", "present_key", "present_value")):
                same_bits(got.numpy(), w, f"replay with seqlens_k {n} ({name})")
    finally:
        ctx.graph_destroy(graph)


# ================================================================================================ graphs: the loader, the executor step, the C-ABI model
from tests.test_gpu_sample import run_cli_graph  # noqa: E402

CLI_MODES = [(), ("--no-fuse",), ("--graph",)]

FORMS = ("rotary_nodes", "do_rotary", "packed")


def gqa_block_case(form, seqlens, batch, seq, past, seed=7, **dims):
    """decoder_block_gqa_graph's feeds and the composition of decoder_rules, gqa_rules and the oracle (matmul_f32) that its outputs must equal bit for bit.
    total_sequence_length is fed as one int32; for "rotary_nodes" every item has the same length (the one-element offset of the RotaryEmbedding nodes)."""
    from oracle import ref
    from rten_amd import onnx_writer as ow
    from tests import decoder_rules as R
    data, w = ow.decoder_block_gqa_graph(form, **dims)
    hidden, heads, kv, d = (dims.get(k, v) for k, v in (("hidden", 64), ("heads", 4), ("kv_heads", 2), ("head_size", 16)))
    seqlens = np.asarray(seqlens, I)
    total = int(seqlens.max()) + 1
    feeds = {"hidden_in": noise(seed, batch, seq, hidden), "residual_in": noise(seed + 1, batch, seq, hidden), "past_k": noise(seed + 2, batch, kv, past, d),
             "past_v": noise(seed + 3, batch, kv, past, d), "seqlens_k": seqlens, "total_sequence_length": np.array([total], I)}
    n1, res1 = R.skip_norm(feeds["hidden_in"], feeds["residual_in"], w["ln1_g"], None, None, 1e-6, True)
    q, k, v = (ref.matmul_f32(n1, w[nm]) for nm in ("wq", "wk", "wv"))
    kw = dict(num_heads=heads, kv_num_heads=kv)
    if form == "rotary_nodes":
        assert len(set(seqlens.tolist())) == 1
        feeds["offset"] = np.array([int(seqlens[0]) + 1 - seq], I)
        q = R.rotary_embedding_microsoft(q, feeds["offset"], w["cos"], w["sin"], False, heads)
        k = R.rotary_embedding_microsoft(k, feeds["offset"], w["cos"], w["sin"], False, kv)
        ctx3, present_k, present_v = G.group_query_attention(q, k, v, feeds["past_k"], feeds["past_v"], seqlens, total, **kw)
    elif form == "do_rotary":
        ctx3, present_k, present_v = G.group_query_attention(q, k, v, feeds["past_k"], feeds["past_v"], seqlens, total, w["cos"], w["sin"], do_rotary=True, **kw)
    else:
        ctx3, present_k, present_v = G.group_query_attention(np.concatenate([q, k, v], axis=2), None, None, feeds["past_k"], feeds["past_v"], seqlens, total, w["cos"],
                                                             w["sin"], do_rotary=True, **kw)
    attn = ref.matmul_f32(ctx3, w["wo"])
    n2, res2 = R.skip_norm(attn, res1, w["ln2_g"], None, None, 1e-6, True)
    gated = (R.silu(ref.matmul_f32(n2, w["w_gate"])) * ref.matmul_f32(n2, w["w_up"])).astype(F)
    want = {"mlp_out": ref.matmul_f32(gated, w["w_down"]), "residual_out": res2, "present_k": present_k, "present_v": present_v}
    return data, feeds, want


_CASES = {}


def shared_gqa_block_case(form):
    """Batch 2 decode on a cache of 3 rows; the forms whose node rotates carry a right-padded item."""
    if form not in _CASES:
        _CASES[form] = gqa_block_case(form, [3, 3] if form == "rotary_nodes" else [3, 2], batch=2, seq=1, past=3)
    return _CASES[form]


@pytest.mark.parametrize("extra", CLI_MODES + [("-t",)], ids=["fused", "unfused", "captured", "node by node"])
@pytest.mark.parametrize("form", FORMS)
def test_decoder_block_gqa_graph_through_the_cli(ctx, tmp_path, form, extra):
    data, feeds, want = shared_gqa_block_case(form)
    got, log = run_cli_graph(tmp_path, data, feeds, list(want), {"batch": 2, "seq": 1, "past": 3}, extra)
    for name, w in want.items():
        same_bits(got[name].reshape(w.shape), w, f"decoder block ({form}) {extra} output {name}")
    if extra == ("--graph",):
        assert "Captured" in log, log[-1500:]
    if extra == ("-t",):
        assert "com.microsoft.GroupQueryAttention" in log, log[-3000:]


def test_a_prompt_chunk_through_the_cli(ctx, tmp_path):
    data, feeds, want = gqa_block_case("do_rotary", [4], batch=1, seq=2, past=3, seed=13)
    got, _ = run_cli_graph(tmp_path, data, feeds, list(want), {"batch": 1, "seq": 2, "past": 3}, ())
    for name, w in want.items():
        same_bits(got[name].reshape(w.shape), w, f"prompt chunk, output {name}")


BIG = dict(hidden=256, heads=4, kv_heads=2, head_size=64, ffn=96)  # head size 64: the one-launch decode kernel


def _bind(ctx, m, feeds):
    from rten_amd.tensor import DeviceTensor
    bound = {}
    for name in m.inputs:
        a = feeds[name]
        bound[name] = DeviceTensor(ctx, a.shape, a.dtype, ptr=m.bind_input(name, a.shape), keepalive=m)
        bound[name].upload(a)
    ctx.sync()
    return bound


def _outputs(ctx, m):
    from rten_amd.tensor import DeviceTensor
    return {name: DeviceTensor(ctx, m.output(i)[1], F, ptr=m.output(i)[0], keepalive=m).numpy() for i, name in enumerate(m.outputs)}


@pytest.mark.parametrize("form", FORMS)
def test_decoder_block_gqa_through_the_c_abi_model_eager_and_captured(ctx, form):
    from rten_amd import lib as L
    # (the C-ABI model gives every input the same dim 0: batch 1, and total_sequence_length bound as [1])
    for dims in ({}, BIG):
        data, feeds, want = gqa_block_case(form, [5], batch=1, seq=1, past=5, seed=9, **dims)
        for captured in (False, True):
            m = L.Model(ctx, data)
            try:
                _bind(ctx, m, feeds)
                if captured:
                    m.prepare()
                    m.run()
                    m.sync()
                else:
                    m.run_eager()
                    ctx.sync()
                got = _outputs(ctx, m)
                for name, w in want.items():
                    same_bits(got[name].reshape(w.shape), w, f"decoder block ({form}, {dims or 'small'}), C-ABI model, captured {captured}, output {name}")
            finally:
                m.close()


@pytest.mark.parametrize("dims", [{}, BIG], ids=["composed", "decode-kernel"])
def test_one_captured_plan_follows_new_device_lengths(ctx, dims):
    """past = 6, S = 1: ONE captured plan replayed with seqlens_k of 2, 3 and 4 written to the model's device inputs; each replay must match the rule, so
    nothing is baked in at capture (the step reads nothing back and is not batch_coupled: the plan captures at all)."""
    from rten_amd import lib as L
    data, feeds, _ = gqa_block_case("do_rotary", [6], batch=1, seq=1, past=6, seed=21, **dims)
    m = L.Model(ctx, data)
    try:
        bound = _bind(ctx, m, feeds)
        m.prepare()
        for n in (2, 3, 4):
            bound["seqlens_k"].upload(np.array([n], I))
            bound["total_sequence_length"].upload(np.array([7], I))
            ctx.sync()
            m.run()
            m.sync()
            got = _outputs(ctx, m)
            _, feeds_n, want = gqa_block_case("do_rotary", [n], batch=1, seq=1, past=6, seed=21, **dims)
            # (the rule is asked total = 7 as the replay is: not a first prompt either way)
            for name, w in want.items():
                same_bits(got[name].reshape(w.shape), w, f"replay with seqlens_k {n}, output {name}")
    finally:
        m.close()


def test_loader_refusals_name_the_node(ctx, tmp_path):
    from rten_amd import onnx_writer as ow
    from tests.test_graph_executor import run_cli
    data, _ = ow.decoder_block_gqa_graph("do_rotary")
    # (every refusal is covered without a device by tests/cpp/test_gqa_hostops.cpp; here: the CLI's exit status and message on real files)
    p = tmp_path / "ok.onnx"
    p.write_bytes(data)
    r = run_cli("--parse-only", str(p))
    assert r.returncode == 0 and 'attention step com.microsoft.GroupQueryAttention "attention": num_heads 4, kv_num_heads 2, separate q / k / v, rotary in halves' in r.stdout, \
        r.stdout[-2000:] + r.stderr[-2000:]
    bad = tmp_path / "bad.onnx"
    bad.write_bytes(ow.decoder_block_gqa_graph("do_rotary", smooth_softmax=1)[0])
    r = run_cli("-s", "batch=1", "-s", "seq=1", "-s", "past=3", str(bad))
    assert r.returncode == 1 and "com.microsoft.GroupQueryAttention attention: smooth_softmax is not supported" in r.stderr, r.stderr
