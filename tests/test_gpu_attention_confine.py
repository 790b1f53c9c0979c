"""What opset-23 Attention's three forms (attention_kv.hip: the decode kernel and the composed path; attention_split.hip) may touch, and what they make of
operands no operator hands them: rten_hip_attention_f32 called with raw strides, every operand and output in a tests/confine.py `Guarded` allocation.

  * every byte outside `out` (its stride gaps included) and outside both presents still holds the fill after the call;
  * input guards and the gaps of strided inputs are NaN: a stray load that reaches an output fails the bit comparison with tests/attention_rules.py;
  * the layouts the header promises beyond (B, H, S, D) and (B, S, H * D), present pointers NULL, non-finite values inside the operands, operands whose
    scores overflow or whose probabilities vanish (the same bands through GroupQueryAttention's decode forms), and the second trip of the three loops that
    work in passes of 64 MiB of scratch.
The cases come from tests/attention_cases.py, whose claims tests/test_attention_cases.py proves on the rules without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import attention_cases as AC
from tests import confine as K
from tests.reduce_rules import same_bits

F, I = np.float32, np.int32
pytestmark = pytest.mark.gpu

AUTO, COMPOSED, DECODE, SPLIT = 0, 1, 2, 3  # rten_hip_set_attention_path
# (path, keys per workgroup of the split form)
FORMS = {"decode": (DECODE, 0), "split8": (SPLIT, 8), "split136": (SPLIT, 136), "composed": (COMPOSED, 0)}
PASS_BYTES = 64 << 20  # SPLIT_PASS_BYTES (attention_split.hip, gqa_split.hip) and SCORE_PASS_BYTES (attention_kv.hip)

_WANT = {}


def expected(case):
    """The rule's [out, present_key, present_value] for a case, computed once and left unchanged."""
    if id(case) not in _WANT:
        _WANT[id(case)] = (case, AC.expected(case))
    return _WANT[id(case)][1]


def guard_bytes(case):
    """One whole [T, max(D, Dv)] head slab in front and behind: a stray store one (batch, KV head) unit off still lands inside."""
    return max(K.GUARD_FLAT, 4 * case.t * max(case.d, case.dv))


def launch(ctx, case, path, split=0, guarded=True, present=(True, True), refused=None):
    """rten_hip_attention_f32 on the case's buffers -> the output allocations (out, present_key, present_value; None where the pointer was NULL).
    refused: the error code the call must return instead of running."""
    from rten_amd import lib as L
    g = guard_bytes(case) if guarded else 0
    guard = lambda a, **kw: K.Guarded(ctx, a, front=g, back=g, **kw)
    bufs = {nm: guard(a) for nm, a in case.bufs.items()}
    ptr = {nm: C.c_void_p(bufs[b].ptr + 4 * off) for nm, (b, off) in case.where.items()}
    opt = lambda a: None if a is None else guard(a)
    pk, pv, mask, nonpad = opt(case.pk), opt(case.pv), opt(case.mask_buf), opt(case.nonpad)
    og = guard(case.o_span * 4, lead=1)
    pkg = guard(case.b * case.hkv * case.t * case.d * 4, lead=2) if present[0] else None
    pvg = guard(case.b * case.hkv * case.t * case.dv * 4, lead=3) if present[1] else None
    dims = (C.c_int32 * 10)(case.b, case.hq, case.hkv, case.sq, case.skv, case.past, case.d, case.dv, int(case.causal), case.mask_kind)
    st = (C.c_int64 * 16)(*case.strides)
    scale = float(F(1.0) / np.sqrt(F(case.d))) if case.scale is None else case.scale
    vp = lambda x: None if x is None else x.vp
    ctx.call("rten_hip_set_attention_path", path)
    ctx.call("rten_hip_set_attention_split", split)
    try:
        code = None
        try:
            ctx.call("rten_hip_attention_f32", dims, st, scale, ptr["q"], ptr["k"], ptr["v"], vp(mask), vp(pk), vp(pv), vp(nonpad), og.vp, vp(pkg), vp(pvg))
        except L.HipError as e:
            if refused is None:
                raise
            code = e.code
        assert code == refused, (code, refused)
        ctx.sync()
    finally:
        ctx.call("rten_hip_set_attention_path", AUTO)
        ctx.call("rten_hip_set_attention_split", 0)
    return og, pkg, pvg


def attend_raw(ctx, case, path, guarded=True, want_present=True, split=0, what=""):
    """The call on guarded operands -> (out (B, Hq, Sq, Dv), present_key, present_value), each confined and bit-equal to the rule."""
    og, pkg, pvg = launch(ctx, case, path, split, guarded, (want_present, want_present))
    want = expected(case)
    what = f"attention {case.name} {what} B {case.b} Hq {case.hq} Hkv {case.hkv} Sq {case.sq} Skv {case.skv} P {case.past} D {case.d} Dv {case.dv} " \
           f"causal {case.causal} path {path} split {split} present {want_present} strides {case.strides}"
    got = [og.check(og.raw(), case.o_shape, (*case.strides[9:12], 1), F, what + " (output)", axes=("batch", "head", "row", "column"))]
    if want_present:
        for alloc, w, width, name in ((pkg, want[1], case.d, "present_key"), (pvg, want[2], case.dv, "present_value")):
            shape = (case.b, case.hkv, case.t, width)
            got.append(alloc.check(alloc.raw(), shape, K.dense(shape), F, f"{what} ({name})", axes=("batch", "KV head", "key", "column")))
            same_bits(got[-1], w, f"{what} ({name})")
    same_bits(got[0], want[0], what + " (output)")
    return got


HEADS = [(4, 4), (8, 2), (16, 1)]
# one new row on a past of T - 1: the 8-key tail, the 64 softmax chunk and the 128 column block, each +-1
TOTALS = [1, 7, 8, 9, 63, 64, 65, 129, 135]


# ================================================================================================ 1. confinement at every length
@pytest.mark.parametrize("heads", HEADS, ids=lambda p: "hq%d-hkv%d" % p)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("form", list(FORMS))
def test_every_path_writes_only_its_outputs(ctx, form, d, heads):
    path, split = FORMS[form]
    hq, hkv = heads
    for i, t in enumerate(TOTALS):  # the layouts alternating
        attend_raw(ctx, AC.standard("one new row", t + d, 2, hq, hkv, 1, 1, t - 1, d, rank=3 + i % 2), path, split=split)
    for rank in (3, 4):
        attend_raw(ctx, AC.standard("three new rows", 6, 2, hq, hkv, 1, 3, 132, d, rank=rank), path, split=split)
        attend_raw(ctx, AC.standard("external cache", 5, 2, hq, hkv, 1, 135, 0, d, rank=rank), path, split=split)


# ================================================================================================ 2. present pointers NULL
@pytest.mark.parametrize("form", ["decode", "split8", "composed"])
def test_present_null_stores_nothing(ctx, form):
    from rten_amd import lib as L
    path, split = FORMS[form]
    for past, skv in ((0, 135), (134, 1), (0, 1)):  # (composed, with a past: K and V are concatenated into scratch; without one and dense: read in place)
        for rank in (3, 4):
            case = AC.standard("present NULL", 11 + past, 2, 8, 2, 1, skv, past, 64, rank=rank)
            wanted = attend_raw(ctx, case, path, split=split)[0]
            alone = attend_raw(ctx, case, path, split=split, want_present=False)[0]
            same_bits(alone, wanted, f"{form} past {past} rank {rank}: the output without present against the output with it")
    if form == "composed":  # more query rows than one: the blocked GEMMs on scratch K / V
        case = AC.standard("present NULL, three rows", 12, 2, 8, 2, 3, 3, 5, 64, rank=3, causal=True)
        same_bits(attend_raw(ctx, case, path, want_present=False)[0], attend_raw(ctx, case, path)[0], "three rows without present")
    case = AC.standard("one present NULL", 13, 2, 8, 2, 1, 1, 40, 64)
    for present in ((True, False), (False, True)):  # refused, and nothing is launched: every output byte still holds the fill
        for alloc in launch(ctx, case, path, split, present=present, refused=L.ERR_INVALID_VALUE):
            assert alloc is None or (alloc.raw() == K.FILL).all(), f"{form}: a refused call wrote to an output"


# ================================================================================================ 3. layouts
@pytest.mark.parametrize("form", list(FORMS))
def test_strided_layouts(ctx, form):
    path, split = FORMS[form]
    shapes = [dict(sq=1, skv=1, past=70)]
    if path == COMPOSED:  # three causal rows: packed-qkv and out-slack take one launch per batch item; bhsd-padded on no past is read out of present / scratch
        shapes += [dict(sq=3, skv=3, past=5, causal=True), dict(sq=3, skv=3, past=0, causal=True)]
    for shape in shapes:
        for case in AC.strided_layouts(2, 8, 2, shape["sq"], shape["skv"], 64, 64, past=shape["past"], causal=shape.get("causal", False)):
            for want_present in (True, False):
                attend_raw(ctx, case, path, split=split, want_present=want_present)


@pytest.mark.parametrize("form", ["decode", "split8", "composed"])
def test_strided_layouts_with_two_head_sizes(ctx, form):
    """D = 128 on the one-workgroup kernel; D = 64 with Dv = 128 where the form takes them (the decode kernel wants D == Dv)."""
    path, split = FORMS[form]
    for d, dv in ((128, 128),) + (() if path == DECODE else ((64, 128),)):
        for case in AC.strided_layouts(2, 4, 2, 1, 1, d, dv, past=64):
            attend_raw(ctx, case, path, split=split)


# ================================================================================================ 4. non-finite values
@pytest.mark.parametrize("form", ["decode", "split8", "composed"])
@pytest.mark.parametrize("name", AC.NONFINITE)
def test_non_finite_values_stay_in_their_heads(ctx, name, form):
    path, split = FORMS[form]
    fin, bad, dep = AC.nonfinite_case(name)
    clean = attend_raw(ctx, fin, path, split=split)
    got = attend_raw(ctx, bad, path, split=split)  # bit-equal to the rule, whose dependency set tests/test_attention_cases.py proves
    same_bits(got[0][~dep["out"]], clean[0][~dep["out"]], f"{name} {form}: outputs outside the dependency set against the finite run")


# ================================================================================================ 5. operand range
@pytest.mark.parametrize("form", ["decode", "split8", "split64", "composed"])
@pytest.mark.parametrize("band", AC.RANGE_BANDS)
def test_wide_range_operands(ctx, band, form):
    path, split = (SPLIT, 64) if form == "split64" else FORMS[form]
    case = AC.range_band(band)
    out = attend_raw(ctx, case, path, split=split)[0]
    ok, figures = AC.band_holds(band, out)  # (follows from the bit comparison; kept so that a failure names the band's figures)
    assert ok, (band, figures)


@pytest.mark.parametrize("path", [2, 3], ids=["decode", "split"])  # rten_hip_set_gqa_path
@pytest.mark.parametrize("band", AC.RANGE_BANDS)
def test_wide_range_operands_through_group_query_attention(ctx, band, path):
    from tests.test_gpu_gqa import gqa
    from tests.test_gpu_gqa_split import keys_per_workgroup
    case = AC.range_band(band)
    q, k, v, pk, pv, seqlens, total, bias = AC.gqa_operands(case)
    for chunk in ((8, 64) if path == 3 else (0,)):
        with keys_per_workgroup(ctx, chunk):
            out = gqa(ctx, q, k, v, pk, pv, seqlens, total, h=case.hq, kv=case.hkv, bias=bias, path=path, what=band)[0]
        ok, figures = AC.band_holds(band, out.reshape(case.b, 1, case.hq, case.dv).transpose(0, 2, 1, 3))
        assert ok, (band, figures)


# ================================================================================================ 6-8. the second trip of the loops over 64 MiB passes
def split_unit_bytes(g, t, dv):
    """attention_split.hip / gqa_split.hip, plan_of: one (batch, KV head) unit's score rows and block sums."""
    return 4 * g * (K.round_up(t, 64) + (t + 7) // 8 * dv)


def test_split_form_second_pass(ctx):
    """B = 2, Hq = 512 on one KV head, T = 1024, Dv = 128: a unit costs 35.7 MB, so a pass holds one unit and item 1 runs in the second (u0 = 1)."""
    b, hq, hkv, d, dv, t = 2, 512, 1, 64, 128, 1024
    unit = split_unit_bytes(hq // hkv, t, dv)
    assert 2 * unit > PASS_BYTES >= unit, unit
    case = AC.standard("second pass", 21, b, hq, hkv, 1, 1, t - 1, d, dv)
    for split in (0, 136):
        attend_raw(ctx, case, SPLIT, split=split)


def test_gqa_split_form_second_pass(ctx):
    """H = 512 on one KV head, D = 128, B = 2 at the shortest cache whose unit is more than half a pass: item 1 runs in the second pass of gqa_split.hip."""
    from tests.test_gpu_gqa import decode_operands, gqa
    b, h, kv, d = 2, 512, 1, 128
    fits = lambda t: 2 * split_unit_bytes(h // kv, t, d) > PASS_BYTES >= split_unit_bytes(h // kv, t, d)
    t = next(t for t in range(1, 4096) if fits(t))
    assert fits(t) and not fits(t - 1) and t == 961, t
    gqa(ctx, *decode_operands(22, b, h, kv, d, t - 1), [t - 1, t - 1], t, h=h, kv=kv, path=3, what="second pass")


@pytest.mark.parametrize("rank", [4, 3])
def test_composed_path_second_pass_over_query_rows(ctx, rank):
    """Hq * Sq * T * 4 = 72 MB of scores: more than the 64 MiB one pass may hold, so the last query rows run in a second pass (s0 > 0).  The 4-D layout
    without present reads K and V in place; the 3-D layout with present goes through the concatenation launch."""
    b, hq, hkv, s, d = 1, 8, 2, 1500, 64
    assert b * hq * s * s * 4 > PASS_BYTES > b * hq * s * s * 2
    case = AC.standard("two passes over the query rows", 24, b, hq, hkv, s, s, 0, d, rank=rank, causal=True)
    attend_raw(ctx, case, COMPOSED, want_present=rank == 3)
