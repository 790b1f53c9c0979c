"""tests/attention_cases.py held to its own claims on the rules alone, before a GPU sees a case: every layout gathers back to its dense operands (and
names no element twice), every non-finite case's dependency set is exact, every range band's predicate holds on tests/attention_rules.py (and, for the
GroupQueryAttention form of the same operands, on tests/gqa_rules.py), and the oracle confines MatMulNBits' non-finite rows and columns."""
import numpy as np
import pytest

from oracle import ref
from tests import attention_cases as AC
from tests import gqa_rules as G
from tests.reduce_rules import canon, same_bits

F = np.float32

# the shapes tests/test_gpu_attention_confine.py::test_strided_layouts runs: one row on a past (the decode forms), three causal rows on a past of 5 and on none
LAYOUT_SHAPES = [dict(sq=1, skv=1, past=70), dict(sq=3, skv=3, past=5, causal=True), dict(sq=3, skv=3, past=0, causal=True)]


@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
def test_every_layout_gathers_back_to_its_dense_operands(shape):
    names = []
    for c in AC.strided_layouts(2, 8, 2, shape["sq"], shape["skv"], 64, 64, past=shape["past"], causal=shape.get("causal", False)):
        names.append(c.name)
        q, k, v, mask = AC.gathered(c)
        for got, want, nm in ((q, c.q, "q"), (k, c.k, "k"), (v, c.v, "v")):
            same_bits(got, want, f"{c.name}: {nm} through its strides")
        if c.mask is not None:
            assert np.array_equal(mask, c.mask), c.name
        # no two elements of the output share an address, and the output fits its region
        at = AC.index(c.o_shape, c.strides[9:12]).reshape(-1)
        assert len(np.unique(at)) == at.size and at.max() + 1 == c.o_span, c.name
        # the rule on the gathered operands is the rule on the dense ones (the layouts change addresses, nothing else)
        assert all(x >= 0 for x in c.strides)
    assert names == ["packed-qkv", "out-slack", "bhsd-padded", "mask-head-and-row-float", "mask-head-and-row-bool"]


def test_the_layouts_leave_what_they_promise():
    by = {c.name: c for c in AC.strided_layouts(2, 8, 2, 3, 3, 64, 64, past=5, causal=True)}
    row = (8 + 2 * 2) * 64
    c = by["packed-qkv"]
    assert list(c.bufs) == ["qkv"] and c.bufs["qkv"].size == 2 * 3 * row and not np.isnan(c.bufs["qkv"]).any()  # q, k, v tile the buffer exactly
    assert c.strides[0:9] == [3 * row, 64, row] * 3 and c.strides[0] != 8 * c.strides[1]  # (not `merged`: one launch per batch item on the composed path)
    c = by["out-slack"]
    assert c.strides[9:12] == [3 * (8 * 64 + 24) + 40, 64, 8 * 64 + 24] and (c.strides[11] * 4) % 16 == 0 and c.strides[11] % 8 == 0
    c = by["bhsd-padded"]
    assert c.strides[3:9] == [2 * (3 * 72 + 16), 3 * 72 + 16, 72] * 2 and np.isnan(c.bufs["k"]).sum() == c.bufs["k"].size - c.k.size
    for kind in ("float", "bool"):
        c = by["mask-head-and-row-" + kind]
        assert c.strides[12] == 0 and c.strides[13] > c.sq * c.strides[14] > 0 and c.strides[14] > c.t and c.strides[15] == 1


def differs(a, b):
    return canon(np.ascontiguousarray(a)) != canon(np.ascontiguousarray(b))


@pytest.mark.parametrize("name", AC.NONFINITE)
def test_every_dependency_set_is_exact(name):
    fin, bad, dep = AC.nonfinite_case(name)
    want_fin, want_bad = AC.expected(fin), AC.expected(bad)
    out = differs(want_bad[0], want_fin[0])[:, :, 0]  # [B, Hq, Dv]
    assert not out[~dep["out"]].any(), f"{name}: an output outside the set changed"
    assert out[dep["out"]].any(axis=-1).all(), f"{name}: an output inside the set did not change"
    for i, key in ((1, "pk"), (2, "pv")):
        rows = differs(want_bad[i], want_fin[i])  # [B, Hkv, T, D]
        assert not rows[~dep[key]].any(), f"{name}: a present row outside the set changed"
        assert rows[dep[key]].all(), f"{name}: a present row inside the set did not change"
    assert dep["out"].any() and not dep["out"].all()


@pytest.mark.parametrize("name", AC.RANGE_BANDS)
def test_every_band_holds_on_the_rules(name):
    c = AC.range_band(name)
    out = AC.expected(c)[0]
    ok, figures = AC.band_holds(name, out)
    assert ok, (name, figures)
    # the same operands as GroupQueryAttention's decode step: its rule's result holds the same predicate
    q, k, v, pk, pv, seqlens, total, bias = AC.gqa_operands(c)
    got = G.group_query_attention(q, k, v, pk, pv, seqlens, total, None, None, None, bias, num_heads=c.hq, kv_num_heads=c.hkv)[0]
    ok, figures = AC.band_holds(name, got.reshape(c.b, 1, c.hq, c.dv).transpose(0, 2, 1, 3))
    assert ok, (name, "GroupQueryAttention", figures)


def test_a_band_that_degenerates_is_noticed():
    c = AC.range_band("one_survivor")
    ordinary = AC.expected(AC.standard("ordinary", 900, c.b, c.hq, c.hkv, 1, 1, c.past, c.d))[0]
    for name in AC.RANGE_BANDS:
        assert not AC.band_holds(name, ordinary)[0], name


def test_the_oracle_confines_matmul_nbits_non_finite_rows_and_columns():
    m, k, n, bs = AC.NBITS_NONFINITE_SHAPE
    lhs, quant, scales = AC.nbits_operands((m,), k, n, bs)
    bad_lhs, bad_scales, dep = AC.nbits_nonfinite(lhs, scales)
    with np.errstate(all="ignore"):
        fin, bad = ref.matmul_nbits_f32(lhs, quant, scales), ref.matmul_nbits_f32(bad_lhs, quant, bad_scales)
    changed = differs(bad, fin)
    assert np.array_equal(changed, dep), f"{(changed != dep).sum()} elements off the dependency set"
    assert np.array_equal(np.flatnonzero(dep.all(axis=1)), [5, m - 1]) and np.array_equal(np.flatnonzero(dep.all(axis=0)), [7, n - 1])
