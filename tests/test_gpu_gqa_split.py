"""The split decode form of GroupQueryAttention (rten_amd/csrc/gqa_split.hip): the key range of one (batch, KV head) spread over workgroups of
rten_hip_set_gqa_split keys, bit for bit against tests/gqa_rules.py whatever the split -- chunks that end before, at and after kv_len, idle workgroups beyond
it, the left-over keys of a column block, the 8-key tail block, groups of more than 8 heads, windows, bias, rotary, rows past the one-workgroup kernel's LDS
bound, one captured call replayed at three device lengths, and what mode 3 and the setter refuse."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import gqa_rules as G
from tests.reduce_rules import same_bits
from tests.test_gpu_gqa import KV_PAIRS, decode_operands, gqa, noise, tables

F, I = np.float32, np.int32
pytestmark = pytest.mark.gpu

AUTO, DECODE, SPLIT = 0, 2, 3  # rten_hip_set_gqa_path


@contextlib.contextmanager
def keys_per_workgroup(ctx, n):
    ctx.call("rten_hip_set_gqa_split", n)
    try:
        yield
    finally:
        ctx.call("rten_hip_set_gqa_split", 0)


@pytest.mark.parametrize("chunk", [8, 64, 136])
@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (16, 1)], ids=lambda p: "h%d-kv%d" % p)
@pytest.mark.parametrize("d", [64, 128])
def test_every_order_at_every_boundary(ctx, d, heads, chunk):
    h, kv = heads
    with keys_per_workgroup(ctx, chunk):
        for a, b in KV_PAIRS:
            past = max(a, b) - 1
            gqa(ctx, *decode_operands(a + d, 2, h, kv, d, past), [a - 1, b - 1], past + 2, h=h, kv=kv, path=SPLIT)
        past = 134
        ops = decode_operands(7, 2, h, kv, d, past)
        gqa(ctx, *ops, [134, 128], 200, h=h, kv=kv, window=4, path=SPLIT)
        gqa(ctx, *ops, [134, 128], 200, h=h, kv=kv, window=200, bias=noise(9, 2, h, 1, past + 3), scale=0.3, path=SPLIT)
        gqa(ctx, *ops, [134, 128], 200, h=h, kv=kv, window=130, bias=noise(10, 1, 1, 2, past + 1), path=SPLIT)


@pytest.mark.parametrize("d", [64, 128])
def test_rotary(ctx, d):
    h, kv, past = 8, 2, 40
    ops = decode_operands(d, 2, h, kv, d, past)
    with keys_per_workgroup(ctx, 8):
        for rot in (d, d // 2):
            cos, sin = tables(rot, 64, rot // 2)
            for interleaved in (False, True):
                gqa(ctx, *ops, [40, 22], 41, h=h, kv=kv, cos=cos, sin=sin, interleaved=interleaved, path=SPLIT)
            gqa(ctx, *ops, [40, 22], 41, h=h, kv=kv, cos=cos, sin=sin, pos=[[63], [5]], path=SPLIT)


def test_rows_past_the_lds_bound(ctx):
    """G = 8, D = 64, 4033 keys: the one-workgroup kernel refuses the row; the split form takes it under mode 3 and under the rule."""
    from rten_amd import lib as L
    h, kv, d, past = 8, 1, 64, 4032
    one, pair = decode_operands(past, 1, h, kv, d, past), decode_operands(past, 2, h, kv, d, past)
    with pytest.raises(L.HipError):
        gqa(ctx, *one, [past], past + 1, h=h, kv=kv, path=DECODE)
    with keys_per_workgroup(ctx, 0):
        gqa(ctx, *one, [past], past + 1, h=h, kv=kv, path=SPLIT)
        gqa(ctx, *pair, [past, past - 5], past + 9, h=h, kv=kv, path=SPLIT, what="right-padded")
        gqa(ctx, *pair, [past, past - 5], past + 9, h=h, kv=kv, path=AUTO, what="right-padded, the rule")


def test_one_captured_launch_replayed_at_three_lengths(ctx):
    """Chunks of 64 keys on a 256-row cache, ONE capture replayed at 63, 64 and 200 keys: nothing is baked in, no counter or scratch is left behind."""
    from rten_amd.tensor import DeviceTensor
    dev = lambda a: DeviceTensor.from_numpy(ctx, np.ascontiguousarray(a))
    h, kv, d, past = 8, 2, 64, 255
    q, k, v, pk, pv = decode_operands(31, 1, h, kv, d, past)
    cos, sin = tables(6, 256, d // 2)
    tq, tk, tv, tpk, tpv, tcos, tsin = (dev(a) for a in (q, k, v, pk, pv, cos, sin))
    seqlens, total = dev(np.array([255], I)), dev(np.array([256], I))
    out, ok, ov = (DeviceTensor(ctx, s, F) for s in ((1, 1, h * d), (1, kv, past + 1, d), (1, kv, past + 1, d)))
    dims = (C.c_int32 * 10)(1, 1, h, kv, d, past, d, 0, 256, 0)
    st = (C.c_int64 * 12)(h * d, h * d, d, kv * d, kv * d, d, kv * d, kv * d, d, 0, 0, 0)

    def launch():
        ctx.call("rten_hip_gqa_f32", dims, st, 0.125, tq.vp, tk.vp, tv.vp, tpk.vp, tpv.vp, seqlens.vp, total.vp, tcos.vp, tsin.vp, None, None, out.vp, ok.vp, ov.vp)

    ctx.call("rten_hip_set_gqa_path", SPLIT)
    try:
        with keys_per_workgroup(ctx, 64):
            launch()  # warm-up: scratch is sized outside the capture
            ctx.sync()
            ctx.graph_begin()
            launch()
            graph = ctx.graph_end()
    finally:
        ctx.call("rten_hip_set_gqa_path", AUTO)
    try:
        for n in (63, 64, 200):
            seqlens.upload(np.array([n - 1], I))
            ctx.graph_launch(graph)
            ctx.sync()
            want = G.group_query_attention(q, k, v, pk, pv, [n - 1], 256, cos, sin, num_heads=h, kv_num_heads=kv, scale=0.125, do_rotary=True)
            for got, w, name in zip((out, ok, ov), want, ("output", "present_key", "present_value")):
                same_bits(got.numpy(), w, f"replay with {n} keys ({name})")
    finally:
        ctx.graph_destroy(graph)


def test_refusals(ctx):
    from rten_amd import lib as L
    with pytest.raises(L.HipError):  # prefill
        gqa(ctx, noise(1, 1, 2, 256), noise(2, 1, 2, 128), noise(3, 1, 2, 128), None, None, [1], 2, h=4, kv=2, path=SPLIT)
    with pytest.raises(L.HipError):  # head size 80
        gqa(ctx, *decode_operands(3, 1, 4, 2, 80, 5), [5], 6, h=4, kv=2, path=SPLIT)
    ctx.call("rten_hip_set_gemv_order", 0, 0)
    try:
        with pytest.raises(L.HipError):
            gqa(ctx, *decode_operands(3, 1, 4, 2, 64, 5), [5], 6, h=4, kv=2, path=SPLIT)
    finally:
        ctx.call("rten_hip_set_gemv_order", 1, 0)
    for bad in (12, -8):
        with pytest.raises(L.HipError):
            ctx.call("rten_hip_set_gqa_split", bad)
    ops = decode_operands(3, 1, 4, 2, 64, 5)
    same_bits(gqa(ctx, *ops, [5], 6, h=4, kv=2)[0], gqa(ctx, *ops, [5], 6, h=4, kv=2, path=DECODE)[0], "automatic path after the refusals")
