"""The fused prefill kernel of opset-23 Attention (rten_amd/csrc/attention_prefill.hip, rten_hip_set_attention_path 4): the output and both presents bit
for bit against tests/attention_rules.py at the strip (64 rows), key-tile (64 keys) and PV depth-block (256 keys) boundaries, every score modification,
its refusals, a cold capture of the no-scratch form, and one float64 check."""
import ctypes as C

import numpy as np
import pytest

from tests import attention_rules as A
from tests.reduce_rules import same_bits
from tests.test_gpu_attention import MODS, attend, noise, operands

F, I = np.float32, np.int32
pytestmark = pytest.mark.gpu

COMPOSED, PREFILL = 1, 4  # rten_hip_set_attention_path

# sq: a partial strip, one strip, a strip boundary; T = past + skv on 63 / 64 / 65 (key tile), 255 / 256 / 257 and 513 (PV fold: two and three depth blocks)
SHAPES = [  # sq, skv, past, d, hq, hkv, rank, causal
    (2, 2, 61, 64, 4, 4, 4, True), (63, 63, 1, 128, 8, 2, 3, False), (64, 64, 1, 64, 16, 1, 4, True), (65, 65, 0, 128, 4, 4, 3, True),
    (130, 130, 0, 64, 8, 2, 4, True), (2, 2, 253, 128, 16, 1, 4, False), (64, 64, 192, 64, 8, 2, 3, True), (65, 65, 192, 128, 8, 2, 4, True),
    (63, 63, 450, 64, 4, 4, 4, True), (130, 130, 383, 128, 8, 2, 3, False),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "sq%d-skv%d-past%d-d%d-hq%d-hkv%d-rank%d-causal%d" % s)
def test_prefill_kernel_at_its_boundaries(ctx, shape):
    sq, skv, past, d, hq, hkv, rank, causal = shape
    attend(ctx, *operands(sq + past + d, 2, hq, hkv, sq, skv, past, d, rank=rank), path=PREFILL, hq=hq, hkv=hkv, is_causal=causal)


PER_ROW = {
    "float mask per row": lambda sq, t: dict(mask=noise(23, 3, 1, sq, t)),
    "bool mask per head and row, item 1 fully masked": lambda sq, t: dict(mask=(np.arange(3)[:, None, None, None] != 1) * (noise(24, 1, 8, sq, t) > -0.5).astype(I)),
    "float mask per row, causal": lambda sq, t: dict(mask=noise(25, 1, 1, sq, t), is_causal=True),
}


@pytest.mark.parametrize("mod", list(MODS) + list(PER_ROW))
def test_score_modifications(ctx, mod):
    sq, t, hq, hkv = 65, 135, 8, 2
    q, k, v, _, _ = operands(30, 3, hq, hkv, sq, t, 0, 64, rank=3)
    kw = MODS[mod](t) if mod in MODS else PER_ROW[mod](sq, t)
    if "nan_row" in kw:
        v.reshape(3, t, hkv, 64)[:, kw.pop("nan_row")] = np.nan  # masked for items 1 and 2: probability 0 times NaN propagates
    attend(ctx, q, k, v, path=PREFILL, hq=hq, hkv=hkv, what=mod, **kw)


def test_causal_nonpad_masks_whole_strips_and_parts_of_others(ctx):
    # item 1: offset 2 - 130: strips 0 and 1 see no key, strip 2 sees one and two; item 0: the plain causal triangle
    attend(ctx, *operands(80, 2, 8, 2, 130, 130, 0, 128), path=PREFILL, nonpad=[130, 2], is_causal=True)


def test_mode_4_gives_mode_1_bits_and_needs_no_present(ctx):
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    hq, hkv = 8, 2
    args = operands(81, 2, hq, hkv, 70, 70, 30, 128, rank=3)
    fused, composed = (attend(ctx, *args, path=path, hq=hq, hkv=hkv, is_causal=True) for path in (PREFILL, COMPOSED))
    same_bits(fused[0], composed[0], "mode 4 against mode 1, outside the rule's range")
    ctx.call("rten_hip_set_attention_path", PREFILL)
    try:  # no present wanted and K / V not readable in place: present goes to scratch
        dev = [None if a is None else DeviceTensor.from_numpy(ctx, a) for a in (*args[:3], None, *args[3:], None)]
        alone = ops.Attention(q_num_heads=hq, kv_num_heads=hkv, is_causal=True).run(ctx, dev, outputs=(0,))[0].numpy()
    finally:
        ctx.call("rten_hip_set_attention_path", 0)
    same_bits(alone, fused[0], "output only")


def test_mode_0_gives_mode_4_bits_inside_the_rule(ctx):
    """A causal first prompt of 2048 rows at head size 64 on 1024 workgroups: the rule's smallest shape.  Device against device: the rule is held above."""
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    dev = [DeviceTensor.from_numpy(ctx, a) for a in operands(82, 1, 32, 8, 2048, 2048, 0, 64)[:3]] + [None] * 4
    got = []
    for path in (0, PREFILL):
        ctx.call("rten_hip_set_attention_path", path)
        try:
            got.append(ops.Attention(is_causal=True).run(ctx, dev, outputs=(0,))[0].numpy())
        finally:
            ctx.call("rten_hip_set_attention_path", 0)
    same_bits(got[0], got[1], "mode 0 against mode 4")


@pytest.mark.parametrize("case", [dict(sq=2, d=80), dict(sq=2, d=64, dv=128), dict(sq=1, d=64)], ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_mode_4_refuses_what_the_kernel_does_not_cover(ctx, case):
    from rten_amd import lib as L
    with pytest.raises(L.HipError):
        attend(ctx, *operands(50, 1, 4, 2, case["sq"], case["sq"], 5, case["d"], case.get("dv")), path=PREFILL)


def test_captured_cold_with_no_scratch_and_replayed_at_two_nonpad_values():
    """Contiguous 4-D inputs, no past, no present: the call allocates nothing, so it is recorded on a context that has launched nothing."""
    from rten_amd import lib as L
    from rten_amd.tensor import DeviceTensor
    b, hq, hkv, d, sq = 2, 8, 2, 64, 70
    q, k, v, _, _ = operands(60, b, hq, hkv, sq, sq, 0, d)
    ctx = L.Context(0)
    try:
        tq, tk, tv = (DeviceTensor.from_numpy(ctx, a) for a in (q, k, v))
        nonpad = DeviceTensor.from_numpy(ctx, np.array([sq, sq], I))
        out = DeviceTensor(ctx, (b, hq, sq, d), F)
        dims = (C.c_int32 * L.ATTENTION_NDIMS)(b, hq, hkv, sq, sq, 0, d, d, 1, L.ATTN_MASK_NONE)
        st = (C.c_int64 * L.ATTENTION_NSTRIDES)(hq * sq * d, sq * d, d, hkv * sq * d, sq * d, d, hkv * sq * d, sq * d, d, hq * sq * d, sq * d, d, 0, 0, 0, 0)
        ctx.call("rten_hip_set_attention_path", PREFILL)
        ctx.sync()
        ctx.graph_begin()
        ctx.call("rten_hip_attention_f32", dims, st, 0.125, tq.vp, tk.vp, tv.vp, None, None, None, nonpad.vp, out.vp, None, None)
        graph = ctx.graph_end()
        for lens in ([70, 3], [1, 65]):
            nonpad.upload(np.array(lens, I))
            for _ in range(2):  # several replays against the eager rule
                ctx.graph_launch(graph)
            ctx.sync()
            same_bits(out.numpy(), A.attention(q, k, v, nonpad_kv_seqlen=lens, is_causal=True, scale=0.125, outputs=(0,))[0], f"replay with nonpad {lens}")
        ctx.graph_destroy(graph)
    finally:
        ctx.close()


def test_against_float64_attention(ctx):
    """Uniform [0, 1) operands and the bound 1e-8 + 1e-5 |want| that tests/test_attention_ops.py holds the rule to."""
    rng = np.random.default_rng(7)
    b, hq, hkv, sq, past, d = 2, 8, 2, 65, 70, 128
    q, k, v = (rng.random(s, dtype=F) for s in ((b, hq, sq, d), (b, hkv, sq, d), (b, hkv, sq, d)))
    pk, pv = rng.random((b, hkv, past, d), dtype=F), rng.random((b, hkv, past, d), dtype=F)
    out, present_k, present_v = attend(ctx, q, k, v, pk, pv, path=PREFILL, is_causal=True)
    want = A.naive(q, present_k, present_v, None, past, None, True, float(F(1.0) / np.sqrt(F(d))))
    assert np.all(np.abs(out - want) <= 1e-8 + 1e-5 * np.abs(want)), np.abs(out - want).max()
