"""The split decode form of opset-23 Attention (rten_amd/csrc/attention_split.hip, mode 3): the key range of one (batch, KV head) spread over workgroups of
rten_hip_set_attention_split keys, the output and both presents bit for bit against tests/attention_rules.py whatever the split -- chunks that end before, at
and after T, a chunk that straddles past and new rows, every score modification, what the one-workgroup kernel refuses (rows past its LDS bound, groups of
more than 32 heads, D != Dv), one captured call replayed with new device nonpad_kv_seqlen, and what mode 3 and the setter refuse."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import attention_rules as A
from tests.reduce_rules import same_bits
from tests.test_gpu_attention import AUTO, DECODE, MODS, TOTALS, attend, noise, operands

F, I = np.float32, np.int32
pytestmark = pytest.mark.gpu

SPLIT = 3  # rten_hip_set_attention_path


@contextlib.contextmanager
def keys_per_workgroup(ctx, n):
    ctx.call("rten_hip_set_attention_split", n)
    try:
        yield
    finally:
        ctx.call("rten_hip_set_attention_split", 0)


@pytest.mark.parametrize("chunk", [8, 64, 136])
@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (16, 1)], ids=lambda p: "hq%d-hkv%d" % p)
@pytest.mark.parametrize("d", [64, 128])
def test_every_order_at_every_boundary(ctx, d, heads, chunk):
    hq, hkv = heads
    with keys_per_workgroup(ctx, chunk):
        for i, t in enumerate(TOTALS):  # one new row appended to a cache of t - 1 rows, the layouts alternating
            attend(ctx, *operands(t + d, 2, hq, hkv, 1, 1, t - 1, d, rank=3 + i % 2), path=SPLIT, hq=hq, hkv=hkv)
        for rank in (3, 4):
            attend(ctx, *operands(5, 2, hq, hkv, 1, 135, 0, d, rank=rank), path=SPLIT, hq=hq, hkv=hkv, what="external cache")
            attend(ctx, *operands(6, 2, hq, hkv, 1, 3, 132, d, rank=rank), path=SPLIT, hq=hq, hkv=hkv, what="three new rows")


@pytest.mark.parametrize("mod", list(MODS))
def test_score_modifications(ctx, mod):
    t, hq, hkv = 135, 8, 2
    q, k, v, _, _ = operands(30, 3, hq, hkv, 1, t, 0, 64, rank=3)
    kw = MODS[mod](t)
    if "nan_row" in kw:
        v.reshape(3, t, hkv, 64)[:, kw.pop("nan_row")] = np.nan  # beyond nonpad for items 1 and 2: probability 0 times NaN propagates, as in the rule
    with keys_per_workgroup(ctx, 8):
        attend(ctx, q, k, v, path=SPLIT, hq=hq, hkv=hkv, what=mod, **kw)
        if mod == "float mask per key":  # with a past, and causal
            attend(ctx, *operands(31, 3, hq, hkv, 1, 1, t - 1, 64), path=SPLIT, is_causal=True, **kw)


@pytest.mark.parametrize("path", [SPLIT, AUTO], ids=["split", "rule"])
@pytest.mark.parametrize("case", [dict(hq=8, hkv=1, t=4033, d=64), dict(hq=64, hkv=1, t=135, d=64), dict(hq=8, hkv=2, t=135, d=64, dv=128),
                                  dict(hq=8, hkv=2, t=135, d=128, dv=64)], ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_what_the_one_workgroup_kernel_refuses(ctx, case, path):
    from rten_amd import lib as L
    ops = operands(case["t"], 1, case["hq"], case["hkv"], 1, 1, case["t"] - 1, case["d"], case.get("dv"))
    if path == SPLIT:
        with pytest.raises(L.HipError):
            attend(ctx, *ops, path=DECODE)
    attend(ctx, *ops, path=path)


def test_one_captured_call_follows_new_device_nonpad(ctx):
    from rten_amd import lib as L
    from rten_amd.tensor import DeviceTensor
    b, hq, hkv, d, t = 2, 8, 2, 64, 70
    q, k, v, _, _ = operands(60, b, hq, hkv, 1, t, 0, d)
    tq, tk, tv = (DeviceTensor.from_numpy(ctx, a) for a in (q, k, v))
    nonpad = DeviceTensor.from_numpy(ctx, np.array([t, t], I))
    out, pk, pv = (DeviceTensor(ctx, s, F) for s in ((b, hq, 1, d), (b, hkv, t, d), (b, hkv, t, d)))
    dims = (C.c_int32 * L.ATTENTION_NDIMS)(b, hq, hkv, 1, t, 0, d, d, 1, L.ATTN_MASK_NONE)
    st = (C.c_int64 * L.ATTENTION_NSTRIDES)(hq * d, d, d, hkv * t * d, t * d, d, hkv * t * d, t * d, d, hq * d, d, d, 0, 0, 0, 0)
    launch = lambda: ctx.call("rten_hip_attention_f32", dims, st, 0.125, tq.vp, tk.vp, tv.vp, None, None, None, nonpad.vp, out.vp, pk.vp, pv.vp)
    ctx.call("rten_hip_set_attention_path", SPLIT)
    try:
        with keys_per_workgroup(ctx, 64):
            launch()  # warm-up: scratch is sized outside the capture
            ctx.sync()
            ctx.graph_begin()
            launch()
            graph = ctx.graph_end()
    finally:
        ctx.call("rten_hip_set_attention_path", AUTO)
    try:
        for lens in ([70, 3], [1, 65], [0, 64]):
            nonpad.upload(np.array(lens, I))
            for _ in range(2):  # several replays against the eager result
                ctx.graph_launch(graph)
            ctx.sync()
            want = A.attention(q, k, v, nonpad_kv_seqlen=lens, is_causal=True, scale=0.125)
            for got, w, name in zip((out, pk, pv), want, ("output", "present_key", "present_value")):
                same_bits(got.numpy(), w, f"replay with nonpad {lens} ({name})")
    finally:
        ctx.graph_destroy(graph)


def test_refusals(ctx):
    from rten_amd import lib as L
    for kw in (dict(sq=2, skv=2, d=64), dict(sq=1, skv=1, d=80)):
        with pytest.raises(L.HipError):
            attend(ctx, *operands(50, 1, 4, 2, kw["sq"], kw["skv"], 5, kw["d"]), path=SPLIT)
    ops64 = operands(51, 2, 8, 2, 1, 1, 40, 64)
    ctx.call("rten_hip_set_gemv_order", 0, 0)
    try:
        with pytest.raises(L.HipError):
            attend(ctx, *ops64, path=SPLIT)
    finally:
        ctx.call("rten_hip_set_gemv_order", 1, 0)
    for bad in (12, -8):
        with pytest.raises(L.HipError):
            ctx.call("rten_hip_set_attention_split", bad)
    same_bits(attend(ctx, *ops64, path=AUTO)[0], attend(ctx, *ops64, path=DECODE)[0], "mode 0 against mode 2 after the refusals")
