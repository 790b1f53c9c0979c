"""Opset-23 Attention with past / present caches on the device (rten_amd/csrc/attention_kv.hip): the output and both presents bit for bit against
tests/attention_rules.py -- the cache-appending decode kernel (mode 2) at every length at which its orders change, the composed path (mode 1), one captured
call replayed with new device nonpad_kv_seqlen, mode 2's refusals, and onnx_writer.attention_graph through the executor."""
import numpy as np
import pytest

from tests import attention_rules as A
from tests.reduce_rules import same_bits
from tests.test_gpu_gqa import KV_PAIRS

F, I = np.float32, np.int32
pytestmark = pytest.mark.gpu

AUTO, COMPOSED, DECODE = 0, 1, 2  # rten_hip_set_attention_path
# total lengths: the 8-key tail and the 128-key column block's left-overs (KV_PAIRS), and the softmax chunk of 64
TOTALS = sorted({t for pair in KV_PAIRS for t in pair} | {63, 64, 65})


def noise(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


def operands(seed, batch, hq, hkv, sq, skv, past, d, dv=None, rank=4):
    """q, k, v, past_k, past_v in the 4-D or the 3-D layout."""
    dv = d if dv is None else dv
    shape = (lambda h, s, w: (batch, h, s, w)) if rank == 4 else (lambda h, s, w: (batch, s, h * w))
    pk, pv = (noise(seed + 3, batch, hkv, past, d), noise(seed + 4, batch, hkv, past, dv)) if past else (None, None)
    return noise(seed, *shape(hq, sq, d)), noise(seed + 1, *shape(hkv, skv, d)), noise(seed + 2, *shape(hkv, skv, dv)), pk, pv


def attend(ctx, q, k, v, pk=None, pv=None, mask=None, nonpad=None, path=DECODE, hq=None, hkv=None, what="", **attrs):
    """ops.Attention on the given path -> (out, present_k, present_v) as numpy, each bit-equal to the rule."""
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    dev = lambda a: None if a is None else DeviceTensor.from_numpy(ctx, np.ascontiguousarray(a))
    if q.ndim == 3:
        attrs = dict(q_num_heads=hq, kv_num_heads=hkv, **attrs)
    ctx.call("rten_hip_set_attention_path", path)
    try:
        got = ops.Attention(**attrs).run(ctx, [dev(q), dev(k), dev(v), dev(mask), dev(pk), dev(pv), dev(None if nonpad is None else np.asarray(nonpad, I))],
                                         outputs=(0, 1, 2))
        got = [g.numpy() for g in got]
    finally:
        ctx.call("rten_hip_set_attention_path", AUTO)
    want = A.attention(q, k, v, mask, pk, pv, nonpad, **attrs)
    for g, w, name in zip(got, want, ("output", "present_key", "present_value")):
        same_bits(g, w, f"attention {what} q {q.shape} k {k.shape} past {None if pk is None else pk.shape[2]} path {path} {attrs} ({name})")
    return got


@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (16, 1)], ids=lambda p: "hq%d-hkv%d" % p)
@pytest.mark.parametrize("d", [64, 128])
def test_decode_kernel_at_every_length(ctx, d, heads):
    hq, hkv = heads
    for i, t in enumerate(TOTALS):  # one new row appended to a cache of t - 1 rows, the layouts alternating
        attend(ctx, *operands(t + d, 2, hq, hkv, 1, 1, t - 1, d, rank=3 + i % 2), hq=hq, hkv=hkv)
    for rank in (3, 4):
        attend(ctx, *operands(5, 2, hq, hkv, 1, 135, 0, d, rank=rank), hq=hq, hkv=hkv, what="external cache")
        attend(ctx, *operands(6, 2, hq, hkv, 1, 3, 132, d, rank=rank), hq=hq, hkv=hkv, what="three new rows")


MODS = {
    "float mask per key": lambda t: dict(mask=noise(20, 3, 1, 1, t)),
    "float mask per head": lambda t: dict(mask=noise(21, 1, 8, 1, 1)),
    "bool mask, item 1 fully masked": lambda t: dict(mask=(np.arange(3)[:, None, None, None] != 1) * (noise(22, 3, 1, 1, t) > -0.5).astype(I)),
    "nonpad": lambda t: dict(nonpad=[t, 5, 0]),
    "nonpad, causal": lambda t: dict(nonpad=[t, 5, 0], is_causal=True),
    "NaN in a masked V row": lambda t: dict(nonpad=[t, 5, 0], nan_row=9),
    "explicit scale": lambda t: dict(scale=0.3),
}


@pytest.mark.parametrize("path", [DECODE, COMPOSED], ids=["decode", "composed"])
@pytest.mark.parametrize("mod", list(MODS))
def test_score_modifications_on_both_paths(ctx, mod, path):
    t, hq, hkv = 135, 8, 2
    q, k, v, _, _ = operands(30, 3, hq, hkv, 1, t, 0, 64, rank=3)
    kw = MODS[mod](t)
    if "nan_row" in kw:
        v.reshape(3, t, hkv, 64)[:, kw.pop("nan_row")] = np.nan  # beyond nonpad for items 1 and 2: probability 0 times NaN propagates, as in the reference
    attend(ctx, q, k, v, path=path, hq=hq, hkv=hkv, what=mod, **kw)
    if mod == "float mask per key":  # with a past, and causal (past_seq anchors the window: every key is visible to the one row)
        attend(ctx, *operands(31, 3, hq, hkv, 1, 1, t - 1, 64), path=path, is_causal=True, **kw)


@pytest.mark.parametrize("case", [dict(sq=3, skv=3, past=5, d=64, is_causal=True), dict(sq=2, skv=4, past=3, d=16, dv=24), dict(sq=1, skv=1, past=130, d=80),
                                  dict(sq=5, skv=5, past=0, d=32, rank=3, is_causal=True)], ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_composed_path_covers_the_rest(ctx, case):
    case = dict(case)
    causal = case.pop("is_causal", False)
    rank = case.pop("rank", 4)
    for r in {rank, 3}:
        attend(ctx, *operands(40, 2, 8, 2, case["sq"], case["skv"], case["past"], case["d"], case.get("dv"), rank=r), path=COMPOSED, hq=8, hkv=2, is_causal=causal)


def test_mode_2_refuses_what_the_kernel_does_not_cover_and_mode_0_takes_it_where_it_does(ctx):
    from rten_amd import lib as L
    for kw in (dict(sq=2, skv=2, d=64), dict(sq=1, skv=1, d=80), dict(sq=1, skv=1, d=64, dv=128)):
        with pytest.raises(L.HipError):
            attend(ctx, *operands(50, 1, 4, 2, kw["sq"], kw["skv"], 5, kw["d"], kw.get("dv")))
    ops64 = operands(51, 2, 8, 2, 1, 1, 40, 64)
    from oracle import ref
    ctx.call("rten_hip_set_gemv_order", 0, 0)
    ref.set_gemv_enabled(False)
    try:
        with pytest.raises(L.HipError):
            attend(ctx, *ops64)
        attend(ctx, *ops64, path=AUTO, what="gemv order off: the blocked order on the composed path")
    finally:
        ctx.call("rten_hip_set_gemv_order", 1, 0)
        ref.set_gemv_enabled(True)
    same_bits(attend(ctx, *ops64, path=AUTO)[0], attend(ctx, *ops64, path=DECODE)[0], "mode 0 against mode 2")


def test_one_captured_call_follows_new_device_nonpad(ctx):
    import ctypes as C
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
    launch()
    ctx.sync()
    ctx.graph_begin()
    launch()
    graph = ctx.graph_end()
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


@pytest.mark.parametrize("extra", [(), ("--graph",)], ids=["fused", "captured"])
@pytest.mark.parametrize("rank", [3, 4])
def test_attention_graph_through_the_executor(ctx, tmp_path, rank, extra):
    from rten_amd import onnx_writer as ow
    from tests.test_gpu_sample import run_cli_graph
    hq, hkv, d, past = 8, 2, 64, 9
    q, k, v, pk, pv = operands(70, 2, hq, hkv, 1, 1, past, d, rank=rank)
    mask = noise(71, 2, 1, 1, past + 1)
    data = ow.attention_graph(hq, hkv, d, rank=rank, mask=ow.FLOAT, is_causal=1)
    feeds = {"q": q, "k": k, "v": v, "attn_mask": mask, "past_k": pk, "past_v": pv}
    kw = dict(q_num_heads=hq, kv_num_heads=hkv) if rank == 3 else {}
    want = dict(zip(("y", "present_k", "present_v"), A.attention(q, k, v, mask, pk, pv, is_causal=True, **kw)))
    got, log = run_cli_graph(tmp_path, data, feeds, list(want), {"batch": 2, "seq": 1, "past": past, "total": past + 1}, extra)
    for name, w in want.items():
        same_bits(got[name].reshape(w.shape), w, f"attention_graph rank {rank} {extra} output {name}")
    if extra:
        assert "Captured" in log, log[-1500:]
