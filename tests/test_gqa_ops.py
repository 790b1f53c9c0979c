"""com.microsoft.GroupQueryAttention without a GPU: the rules file (tests/gqa_rules.py) against the reference's own tests -- its five seeded cases regenerated
in its draw order and held to a naive k-ordered float formula at its bar (expect_equal: |x - y| <= 1e-8 + 1e-5 |y|, rten-tensor/src/test_util.rs:47-68), the
present-cache literal, packed QKV, every error string, the output mask -- then the properties the device tests rely on (right padding, windows, bias broadcast,
NaN confinement), the header / bindings / registry additions, and the Python operator on a recording context (launch arguments, refusals before any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ref
from tests import gqa_rules as G
from tests.reduce_rules import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32


def expect_equal(got, want, what):
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want) - (1e-8 + 1e-5 * np.abs(want))
    assert float(err.max(initial=-1.0)) <= 0.0, (what, float(np.abs(got - want).max()))


# (num_heads, kv_num_heads, seq, past_seq, batch, scale): test_group_query_attention (contrib.rs:1013-1059)
CASES = [(2, 2, 4, 0, 1, None), (4, 2, 3, 0, 1, 0.3), (4, 1, 1, 5, 1, None), (4, 2, 3, 2, 1, None), (2, 1, 3, 0, 2, None)]


def seeded_case(h, kv, seq, past, batch, d=8):
    """The draws of the reference's test, in its order: query, key, value, past_key, past_value from XorShiftRng(1234)."""
    rng = ref.XorShiftRng(1234)
    q = rng.f32(batch * seq * h * d).reshape(batch, seq, h * d)
    k = rng.f32(batch * seq * kv * d).reshape(batch, seq, kv * d)
    v = rng.f32(batch * seq * kv * d).reshape(batch, seq, kv * d)
    pk = pv = None
    if past:
        pk = rng.f32(batch * kv * past * d).reshape(batch, kv, past, d)
        pv = rng.f32(batch * kv * past * d).reshape(batch, kv, past, d)
    return q, k, v, pk, pv


@pytest.mark.parametrize("case", CASES, ids=lambda c: "h%d-kv%d-s%d-p%d-b%d" % c[:5])
def test_rule_meets_the_reference_s_bar_on_its_five_seeded_cases(case):
    h, kv, seq, past, batch, scale = case
    q, k, v, pk, pv = seeded_case(h, kv, seq, past, batch)
    total = past + seq
    out, present_k, present_v = G.group_query_attention(q, k, v, pk, pv, np.full(batch, total - 1, I), total, num_heads=h, kv_num_heads=kv, scale=scale)
    want = G.naive(q, k, v, pk, pv, h, kv, scale if scale is not None else float(F(1.0) / np.sqrt(F(8))))
    expect_equal(out, want, str(case))
    assert out.shape == (batch, seq, h * 8) and present_k.shape == present_v.shape == (batch, kv, total, 8)


def test_present_cache_literal():
    """test_group_query_attention_present_cache (contrib.rs:1133-1166)."""
    key = np.arange(1, 9, dtype=F).reshape(1, 1, 8)
    value = np.arange(8, 0, -1, dtype=F).reshape(1, 1, 8)
    past_value = np.arange(16, dtype=F).reshape(1, 1, 2, 8)
    out = G.group_query_attention(np.zeros((1, 1, 16), F), key, value, np.zeros((1, 1, 2, 8), F), past_value, [2], 3, num_heads=2, kv_num_heads=1, scale=1.0)
    assert out[1][0, 0].tolist() == [[0.0] * 8, [0.0] * 8, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]]
    assert out[2][0, 0].tolist() == [list(map(float, range(8))), list(map(float, range(8, 16))), [8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0]]


def test_packed_qkv_equals_separate_bit_for_bit():
    h, kv, d, seq = 4, 2, 8, 3
    packed = ref.XorShiftRng(1234).f32(seq * (h + 2 * kv) * d).reshape(1, seq, (h + 2 * kv) * d)
    q, k, v = packed[:, :, :h * d].copy(), packed[:, :, h * d:(h + kv) * d].copy(), packed[:, :, (h + kv) * d:].copy()
    a = G.group_query_attention(packed, None, None, None, None, [seq - 1], seq, num_heads=h, kv_num_heads=kv)
    b = G.group_query_attention(q, k, v, None, None, [seq - 1], seq, num_heads=h, kv_num_heads=kv)
    assert a[0].shape == (1, seq, h * d)
    for x, y in zip(a, b):
        same_bits(x, y, "packed against separate")


def _zeros_case(seq=2):
    return np.zeros((1, seq, 16), F), np.zeros((1, seq, 8), F), np.zeros((1, seq, 8), F)


def _raises(kind, msg, *args, **kw):
    with pytest.raises(G.OpError) as e:
        G.group_query_attention(*args, **kw)
    assert (e.value.kind, e.value.msg) == (kind, msg), (e.value.kind, e.value.msg)


def test_rejects_unsupported_with_the_reference_s_strings():
    """test_group_query_attention_rejects_unsupported (contrib.rs:1221-1303)."""
    q, k, v = _zeros_case()
    kw = dict(num_heads=2, kv_num_heads=1)
    _raises("UnsupportedValue", "smooth_softmax is not supported", q, k, v, None, None, [1], 2, smooth_softmax=True, **kw)
    _raises("InvalidValue", "num_heads must be a multiple of kv_num_heads", q, k, v, None, None, [1], 2, num_heads=3, kv_num_heads=2)
    _raises("InvalidValue", "seqlens_k entry is too small for the query sequence length", q, k, v, None, None, [0], 1, **kw)
    _raises("InvalidValue", "seqlens_k entry is too small for the query sequence length", q, k, v, None, None, [0], 2, **kw)
    q1, k1, v1 = _zeros_case(1)
    past = np.zeros((1, 1, 2, 8), F)
    _raises("InvalidValue", "seqlens_k entry is out of range", q1, k1, v1, past, past, [9], 10, **kw)
    _raises("UnsupportedValue", "head_sink is not supported", q, k, v, None, None, [1], 2, head_sink=np.zeros(2, F), **kw)


def test_validates_attention_bias():
    """test_group_query_attention_validates_attention_bias (contrib.rs:1345-1405)."""
    q, k, v = _zeros_case()
    kw = dict(num_heads=2, kv_num_heads=1)
    G.group_query_attention(q, k, v, None, None, [1], 2, attention_bias=np.zeros((1, 1, 2, 2), F), **kw)
    for shape in ((1, 1, 1, 2), (1, 1, 2, 1), (1, 3, 2, 2)):
        _raises("IncompatibleInputShapes", "attention_bias shape is incompatible with query/key shapes", q, k, v, None, None, [1], 2,
                attention_bias=np.zeros(shape, F), **kw)


def test_shape_checks_of_contrib_rs():
    q, k, v = _zeros_case()
    kw = dict(num_heads=2, kv_num_heads=1)
    past = np.zeros((1, 1, 2, 8), F)
    _raises("InvalidValue", "num_heads and kv_num_heads must be positive", q, k, v, None, None, [1], 2, num_heads=0, kv_num_heads=1)
    _raises("IncompatibleInputShapes", "query hidden size must be divisible by num_heads", q, k, v, None, None, [1], 2, num_heads=3, kv_num_heads=1)
    _raises("IncompatibleInputShapes", "key and value batch size must match query", q, np.zeros((2, 2, 8), F), np.zeros((2, 2, 8), F), None, None, [1], 2, **kw)
    _raises("IncompatibleInputShapes", "key and value must have the same shape", q, k, np.zeros((1, 2, 16), F), None, None, [1], 2, **kw)
    _raises("IncompatibleInputShapes", "key hidden size must equal kv_num_heads * head_size", q, np.zeros((1, 2, 16), F), np.zeros((1, 2, 16), F), None, None, [1], 2, **kw)
    _raises("UnsupportedValue", "key sequence length must match query sequence length", q, np.zeros((1, 3, 8), F), np.zeros((1, 3, 8), F), None, None, [1], 2, **kw)
    _raises("IncompatibleInputShapes", "packed query hidden size must be divisible by num_heads + 2 * kv_num_heads", np.zeros((1, 2, 30), F), None, None, None, None, [1], 2, **kw)
    _raises("InvalidValue", "key and value must both be present or both absent", q, k, None, None, None, [1], 2, **kw)
    _raises("IncompatibleInputShapes", "seqlens_k must have batch_size elements", q, k, v, None, None, [1, 1], 2, **kw)
    _raises("UnsupportedValue", "seqlens_k must be a vector", q, k, v, None, None, np.zeros((1, 2), I), 2, **kw)
    _raises("InvalidValue", "total_sequence_length must be positive", q, k, v, None, None, [1], 0, **kw)
    _raises("IncompatibleInputShapes", "past_key/past_value shape does not match", q, k, v, past, np.zeros((1, 1, 3, 8), F), [3], 4, **kw)
    _raises("InvalidValue", "past_key and past_value must both be present or both absent", q, k, v, past, None, [3], 4, **kw)
    q2, k2, v2 = np.zeros((2, 2, 16), F), np.zeros((2, 2, 8), F), np.zeros((2, 2, 8), F)
    past2 = np.zeros((2, 1, 2, 8), F)
    _raises("UnsupportedValue", "batch size must be 1 when sequence_length > 1 and a past context is given", q2, k2, v2, past2, past2, [3, 3], 4, **kw)
    _raises("InvalidValue", "cos_cache and sin_cache are required when do_rotary is set", q, k, v, None, None, [1], 2, do_rotary=True, **kw)
    out = G.group_query_attention(q, k, v, None, None, np.array([[1]], I), 2, **kw)  # [B, 1] is accepted
    assert len(out) == 3


def test_output_mask():
    """test_group_query_attention_omits_unrequested_kv_cache (contrib.rs:1305-1343)."""
    q, k, v = _zeros_case()
    kw = dict(num_heads=2, kv_num_heads=1)
    assert len(G.group_query_attention(q, k, v, None, None, [1], 2, outputs=(0,), **kw)) == 1
    assert len(G.group_query_attention(q, k, v, None, None, [1], 2, outputs=(0, 1), **kw)) == 3


def _decode_case(seed, batch, h, kv, d, past):
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.standard_normal(s).astype(F)
    return r(batch, 1, h * d), r(batch, 1, kv * d), r(batch, 1, kv * d), r(batch, kv, past, d), r(batch, kv, past, d)


def test_right_padded_batch_leaves_zero_rows_and_drops_past_rows():
    q, k, v, pk, pv = _decode_case(1, 2, 4, 2, 8, 6)
    out, present_k, present_v = G.group_query_attention(q, k, v, pk, pv, [6, 3], 7, num_heads=4, kv_num_heads=2)
    for present, past, new in ((present_k, pk, k), (present_v, pv, v)):
        same_bits(present[0, :, :6], past[0], "batch 0 keeps its whole past")
        same_bits(present[1, :, :3], past[1, :, :3], "batch 1 keeps three rows")
        same_bits(present[1, :, 3], new[1, 0].reshape(2, 8), "the new token lands at past_len")
        assert not present[1, :, 4:].any()  # the dropped rows of past and the tail stay zero
    # batch 1 equals the same item run alone on its unpadded past
    alone = G.group_query_attention(q[1:], k[1:], v[1:], pk[1:, :, :3], pv[1:, :, :3], [3], 4, num_heads=4, kv_num_heads=2)[0]
    same_bits(out[1:], alone, "a right-padded item")


def test_window_smaller_equal_and_larger_than_the_limit():
    q, k, v, pk, pv = _decode_case(2, 1, 2, 1, 8, 9)  # lim = 10
    full = G.group_query_attention(q, k, v, pk, pv, [9], 10, num_heads=2, kv_num_heads=1)[0]
    for window in (10, 11, 200):
        same_bits(G.group_query_attention(q, k, v, pk, pv, [9], 10, num_heads=2, kv_num_heads=1, local_window_size=window)[0], full, f"window {window} >= lim")
    small = G.group_query_attention(q, k, v, pk, pv, [9], 10, num_heads=2, kv_num_heads=1, local_window_size=4)[0]
    assert not np.array_equal(small, full)
    # a window of 4 sees the last three rows of past and the new token: with the first six rows of past changed, nothing moves
    pk2, pv2 = pk.copy(), pv.copy()
    pk2[:, :, :6], pv2[:, :, :6] = 7.0, -3.0
    same_bits(G.group_query_attention(q, k, v, pk2, pv2, [9], 10, num_heads=2, kv_num_heads=1, local_window_size=4)[0], small, "outside the window")
    assert G.read_attrs({"num_heads": 2, "kv_num_heads": 1, "local_window_size": -1})["local_window_size"] is None
    assert G.read_attrs({"num_heads": 2, "kv_num_heads": 1, "local_window_size": 0})["local_window_size"] is None
    assert G.read_attrs({"num_heads": 2, "kv_num_heads": 1}) == dict(num_heads=2, kv_num_heads=1, scale=None, do_rotary=False, rotary_interleaved=False,
                                                                     local_window_size=None, softcap=0.0, smooth_softmax=False)


def test_bias_broadcast_over_batch_and_head():
    q, k, v, pk, pv = _decode_case(3, 2, 4, 2, 8, 5)
    bias = np.random.default_rng(4).standard_normal((1, 1, 1, 6)).astype(F)
    a = G.group_query_attention(q, k, v, pk, pv, [5, 5], 6, attention_bias=bias, num_heads=4, kv_num_heads=2)[0]
    b = G.group_query_attention(q, k, v, pk, pv, [5, 5], 6, attention_bias=np.ascontiguousarray(np.broadcast_to(bias, (2, 4, 1, 6))), num_heads=4, kv_num_heads=2)[0]
    same_bits(a, b, "broadcast bias")
    assert not np.array_equal(a, G.group_query_attention(q, k, v, pk, pv, [5, 5], 6, num_heads=4, kv_num_heads=2)[0])


def test_nan_in_a_key_row_beyond_a_query_s_causal_limit_is_confined():
    rng = np.random.default_rng(5)
    r = lambda *s: rng.standard_normal(s).astype(F)
    q, k, v = r(1, 4, 16), r(1, 4, 8), r(1, 4, 8)
    clean = G.group_query_attention(q, k, v, None, None, [3], 4, num_heads=2, kv_num_heads=1)[0]
    k2 = k.copy()
    k2[0, 2] = np.nan  # key row 2: queries 0 and 1 end before it
    got = G.group_query_attention(q, k2, v, None, None, [3], 4, num_heads=2, kv_num_heads=1)[0]
    same_bits(got[:, :2], clean[:, :2], "queries before the NaN row")
    assert not np.array_equal(got[:, 2:], clean[:, 2:])


def test_rotary_positions_default_to_past_len_plus_s():
    rng = np.random.default_rng(6)
    r = lambda *s: rng.standard_normal(s).astype(F)
    q, k, v, pk, pv = r(1, 3, 32), r(1, 3, 16), r(1, 3, 16), r(1, 1, 2, 16), r(1, 1, 2, 16)
    cos, sin = r(8, 4), r(8, 4)  # rotary_dim 8 of a head of 16
    kw = dict(num_heads=2, kv_num_heads=1, do_rotary=True)
    a = G.group_query_attention(q, k, v, pk, pv, [4], 5, cos, sin, **kw)
    b = G.group_query_attention(q, k, v, pk, pv, [4], 5, cos, sin, np.array([[2, 3, 4]], I), **kw)
    for x, y in zip(a, b):
        same_bits(x, y, "explicit ids")
    same_bits(a[2][0, 0, 2:], v[0], "V is not rotated")
    assert not np.array_equal(a[1][0, 0, 2:], k[0])
    _raises("InvalidValue", "Entry in `indices` is out of range", q, k, v, pk, pv, [4], 5, cos, sin, np.array([[2, 3, 8]], I), **kw)


# ---------------------------------------------------------------------------------------------- header, bindings, registry
def test_header_bindings_and_registry():
    from rten_amd import lib as L
    from rten_amd import ops
    header = open(os.path.join(ROOT, "include", "rten_hip.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "rten-hip-sys", "src", "lib.rs")).read()
    assert "#define RTEN_HIP_ABI_VERSION 8\n" in header
    for sym, nargs in (("rten_hip_gqa_f32", 18), ("rten_hip_set_gqa_path", 2)):
        assert re.search(r"int32_t " + sym + r"\(", header), sym
        assert sym in L.PROTOTYPES and L.PROTOTYPES[sym][0] is C.c_int32 and len(L.PROTOTYPES[sym][1]) == nargs, sym
        assert f"pub fn {sym}(" in bindings and hasattr(L.load(), sym), sym
    assert (L.GQA_NDIMS, L.GQA_NSTRIDES) == tuple(int(re.search(rf"#define RTEN_HIP_GQA_{k} (\d+)", header).group(1)) for k in ("NDIMS", "NSTRIDES"))
    assert "src/ops/attention/contrib.rs:359-878" in header
    assert "GroupQueryAttention" in ops.OpRegistry.with_all_ops().op_types()
    op = ops.GroupQueryAttention(8, 2)
    assert op.name() == "com.microsoft.GroupQueryAttention" and (op.max_inputs(), op.max_outputs()) == (12, 3)
    assert (op.scale, op.do_rotary, op.rotary_interleaved, op.local_window_size, op.softcap, op.smooth_softmax) == (None, False, False, None, 0.0, False)
    assert ops.GroupQueryAttention(8, 2, local_window_size=0).local_window_size is None and ops.GroupQueryAttention(8, 2, local_window_size=5).local_window_size == 5
    with pytest.raises(TypeError):
        ops.GroupQueryAttention()  # num_heads and kv_num_heads are required (onnx_registry.rs:1468-1469)


# ---------------------------------------------------------------------------------------------- the Python operator on a recording context
def _recording():
    from rten_amd.recording import RecordingCtx

    class Ctx(RecordingCtx):
        def __init__(self):
            super().__init__()
            self.calls = []

        def call(self, name, *args):
            self.calls.append((name, args))
            super().call(name, *args)

    return Ctx()


def _launches(ctx):
    return [(name, args) for name, args in ctx.calls if not name.startswith("rten_hip_mem") and name not in ("rten_hip_malloc", "rten_hip_free")]


def test_python_operator_launch_arguments_and_output_mask():
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    ctx = _recording()
    t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
    B, H, KV, D, P = 2, 8, 2, 64, 5
    q, k, v, pk, pv = t(B, 1, H * D), t(B, 1, KV * D), t(B, 1, KV * D), t(B, KV, P, D), t(B, KV, P, D)
    seqlens, total, cos, sin = t(B, dtype=I), t(dtype=I), t(32, 16), t(32, 16)
    op = ops.GroupQueryAttention(H, KV, do_rotary=True, local_window_size=7)
    outs = op.run(ctx, [q, k, v, pk, pv, seqlens, total, cos, sin])
    assert [tuple(o.shape) for o in outs] == [(B, 1, H * D), (B, KV, P + 1, D), (B, KV, P + 1, D)]
    (name, a), = _launches(ctx)
    assert name == "rten_hip_gqa_f32"
    assert list(a[0]) == [B, 1, H, KV, D, P, 32, 0, 32, 7]
    assert list(a[1]) == [H * D, H * D, D, KV * D, KV * D, D, KV * D, KV * D, D, 0, 0, 0]
    assert abs(a[2] - 0.125) < 1e-9
    assert [x.value for x in a[3:10]] == [q.ptr, k.ptr, v.ptr, pk.ptr, pv.ptr, seqlens.ptr, total.ptr]
    assert [x.value for x in a[10:12]] == [cos.ptr, sin.ptr] and a[12] is None and a[13] is None
    assert [x.value for x in a[14:]] == [o.ptr for o in outs]
    assert len(op.run(ctx, [q, k, v, pk, pv, seqlens, total, cos, sin], outputs=(0,))) == 1
    # packed QKV: three pointers into one buffer, one stride set
    ctx.calls.clear()
    packed = t(B, 1, (H + 2 * KV) * D)
    ops.GroupQueryAttention(H, KV).run(ctx, [packed, None, None, pk, pv, seqlens, total])
    (name, a), = _launches(ctx)
    row = (H + 2 * KV) * D
    assert list(a[1])[:9] == [row, row, D] * 3 and list(a[0])[6:] == [0, 0, 0, 0]
    assert [x.value for x in a[3:6]] == [packed.ptr, packed.ptr + 4 * H * D, packed.ptr + 4 * (H + KV) * D]


def test_python_operator_refuses_with_the_reference_s_strings_before_any_launch():
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor

    def refused(kind, msg, build, **attrs):
        ctx = _recording()
        t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
        attrs = {"num_heads": 2, "kv_num_heads": 1, **attrs}
        with pytest.raises(ops.OpError) as e:
            ops.GroupQueryAttention(**attrs).run(ctx, build(t))
        assert _launches(ctx) == []
        assert (e.value.kind, e.value.msg) == (kind, msg), (e.value.kind, e.value.msg)

    one, two = np.array([1], I), np.array(2, I)
    base = lambda t: [t(1, 2, 16), t(1, 2, 8), t(1, 2, 8), None, None, one, two]
    refused("UnsupportedValue", "smooth_softmax is not supported", base, smooth_softmax=True)
    refused("UnsupportedValue", "head_sink is not supported", lambda t: base(t) + [None] * 4 + [t(2)])
    refused("InvalidValue", "num_heads must be a multiple of kv_num_heads", base, num_heads=3, kv_num_heads=2)
    refused("InvalidValue", "num_heads and kv_num_heads must be positive", base, num_heads=0)
    refused("IncompatibleInputShapes", "query hidden size must be divisible by num_heads", base, num_heads=3)
    refused("IncompatibleInputShapes", "key and value batch size must match query", lambda t: [t(1, 2, 16), t(2, 2, 8), t(2, 2, 8), None, None, one, two])
    refused("IncompatibleInputShapes", "key and value must have the same shape", lambda t: [t(1, 2, 16), t(1, 2, 8), t(1, 2, 16), None, None, one, two])
    refused("IncompatibleInputShapes", "key hidden size must equal kv_num_heads * head_size", lambda t: [t(1, 2, 16), t(1, 2, 16), t(1, 2, 16), None, None, one, two])
    refused("UnsupportedValue", "key sequence length must match query sequence length", lambda t: [t(1, 2, 16), t(1, 3, 8), t(1, 3, 8), None, None, one, two])
    refused("IncompatibleInputShapes", "packed query hidden size must be divisible by num_heads + 2 * kv_num_heads", lambda t: [t(1, 2, 30), None, None, None, None, one, two])
    refused("InvalidValue", "key and value must both be present or both absent", lambda t: [t(1, 2, 16), t(1, 2, 8), None, None, None, one, two])
    refused("IncompatibleInputShapes", "seqlens_k must have batch_size elements", lambda t: base(t)[:5] + [np.array([1, 1], I), two])
    refused("UnsupportedValue", "seqlens_k must be a vector", lambda t: base(t)[:5] + [np.zeros((1, 2), I), two])
    refused("InvalidValue", "total_sequence_length must be positive", lambda t: base(t)[:6] + [np.array(0, I)])
    refused("IncompatibleInputShapes", "past_key/past_value shape does not match", lambda t: base(t)[:3] + [t(1, 1, 2, 8), t(1, 1, 3, 8), np.array([3], I), np.array(4, I)])
    refused("InvalidValue", "past_key and past_value must both be present or both absent", lambda t: base(t)[:3] + [t(1, 1, 2, 8), None, np.array([3], I), np.array(4, I)])
    refused("UnsupportedValue", "batch size must be 1 when sequence_length > 1 and a past context is given",
            lambda t: [t(2, 2, 16), t(2, 2, 8), t(2, 2, 8), t(2, 1, 2, 8), t(2, 1, 2, 8), np.array([3, 3], I), np.array(4, I)])
    # the three value errors of host seqlens_k (contrib.rs:630-639)
    refused("InvalidValue", "seqlens_k entry is too small for the query sequence length", lambda t: base(t)[:5] + [np.array([0], I), np.array(1, I)])
    refused("InvalidValue", "seqlens_k entry is too small for the query sequence length", lambda t: base(t)[:5] + [np.array([0], I), two])
    refused("InvalidValue", "seqlens_k entry is out of range",
            lambda t: [t(1, 1, 16), t(1, 1, 8), t(1, 1, 8), t(1, 1, 2, 8), t(1, 1, 2, 8), np.array([9], I), np.array(10, I)])
    refused("InvalidValue", "seqlens_k entry is out of range", lambda t: base(t)[:5] + [np.array([-1], I), two])
    for shape in ((1, 1, 1, 2), (1, 1, 2, 1), (1, 3, 2, 2)):
        refused("IncompatibleInputShapes", "attention_bias shape is incompatible with query/key shapes", lambda t: base(t) + [None, None, None, t(*shape)])
    refused("InvalidValue", "cos_cache and sin_cache are required when do_rotary is set", base, do_rotary=True)
    refused("UnsupportedValue", "softcap is not supported", base, softcap=30.0)
    # device seqlens_k / total: nothing to validate on the host, the kernels clamp
    ctx = _recording()
    t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
    outs = ops.GroupQueryAttention(2, 1).run(ctx, [t(1, 2, 16), t(1, 2, 8), t(1, 2, 8), None, None, t(1, 1, dtype=I), t(dtype=I)])
    assert len(outs) == 3 and [n for n, _ in _launches(ctx)] == ["rten_hip_gqa_f32"]


# ---------------------------------------------------------------------------------------------- the builder graphs through the loader's device-free checks
@pytest.mark.parametrize("form", ["rotary_nodes", "do_rotary", "packed"])
def test_builder_graphs_pass_the_loader_s_parse_only_checks(tmp_path, form):
    from rten_amd import onnx_writer as ow
    from tests.test_graph_executor import run_cli
    data, w = ow.decoder_block_gqa_graph(form, local_window_size=5 if form == "packed" else -1)
    base, wb = ow.decoder_block_graph()
    assert sorted(w) == sorted(wb) and all(np.array_equal(w[k], wb[k]) for k in w)  # the same weights as the composed block
    p = tmp_path / (form + ".onnx")
    p.write_bytes(data)
    r = run_cli("--parse-only", str(p))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if "attention step com.microsoft.GroupQueryAttention" in ln]
    assert len(line) == 1 and "num_heads 4, kv_num_heads 2" in line[0] and "present caches read" in line[0], r.stdout
    assert ("packed QKV" in line[0]) == (form == "packed") and ("rotary off" in line[0]) == (form == "rotary_nodes")
    assert ("window 5" in line[0]) == (form == "packed")


def test_parse_only_refuses_by_node_name(tmp_path):
    from rten_amd import onnx_writer as ow
    from tests.test_graph_executor import run_cli
    for attrs, words in ((dict(smooth_softmax=1), "smooth_softmax is not supported"), (dict(softcap=30.0), "softcap != 0 is not supported")):
        p = tmp_path / "bad.onnx"
        p.write_bytes(ow.decoder_block_gqa_graph("do_rotary", **attrs)[0])
        r = run_cli("--parse-only", str(p))
        assert r.returncode == 1 and "com.microsoft.GroupQueryAttention attention: " + words in r.stderr, r.stdout[-1500:] + r.stderr[-1500:]
