"""Opset-23 Attention without a device: tests/attention_rules.py against a float64 numpy attention (the bound is the one tests/test_gqa_ops.py holds its rule
to: 1e-8 + 1e-5 |want|), the reference's error strings from the rule and from the Python operator, and the loader's device-free checks on
onnx_writer.attention_graph."""
import numpy as np
import pytest

from tests import attention_rules as A
from tests.test_gqa_ops import _recording, expect_equal

F, I = np.float32, np.int32


def noise(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


def unit(seed, *shape):
    """Uniform [0, 1) draws, as the reference's attention tests and tests/test_gqa_ops.py make them: the bound taken from there is relative to |want|, which
    suits sums without cancellation (an output is a convex combination of V rows of one sign)."""
    return np.random.default_rng(seed).random(shape, dtype=F)


# rank, Hq, Hkv, Sq, Skv, past, D, Dv, then mask kind / causal / nonpad
CASES = [dict(rank=4, sq=3, skv=3, past=0), dict(rank=3, sq=1, skv=1, past=9, causal=True), dict(rank=4, sq=2, skv=2, past=5, causal=True, mask="float"),
         dict(rank=3, sq=3, skv=7, past=0, mask="bool"), dict(rank=4, sq=1, skv=12, past=0, nonpad=[12, 5, 0]),
         dict(rank=3, sq=3, skv=12, past=0, nonpad=[12, 5, 0], causal=True), dict(rank=4, sq=2, skv=4, past=3, dv=24), dict(rank=4, sq=1, skv=140, past=0)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items() if k != "nonpad"))
def test_rule_against_float64_attention(case):
    b, hq, hkv, d = 3, 4, 2, 16
    sq, skv, past, dv, rank = case["sq"], case["skv"], case["past"], case.get("dv", 16), case["rank"]
    t = past + skv
    q4, k4, v4 = unit(1, b, hq, sq, d), unit(2, b, hkv, skv, d), unit(3, b, hkv, skv, dv)
    pk, pv = (unit(4, b, hkv, past, d), unit(5, b, hkv, past, dv)) if past else (None, None)
    mask = {None: None, "float": noise(6, b, 1, sq, t), "bool": (noise(7, 1, hq, 1, t) > 0).astype(I)}[case.get("mask")]
    if mask is not None and mask.dtype == I:
        mask[0, 1] = 0  # a fully masked row: zeros
    merge = lambda x: np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(b, x.shape[2], -1)
    ins = (q4, k4, v4) if rank == 4 else (merge(q4), merge(k4), merge(v4))
    kw = dict(q_num_heads=hq, kv_num_heads=hkv) if rank == 3 else {}
    out, present_k, present_v = A.attention(*ins, mask, pk, pv, case.get("nonpad"), is_causal=case.get("causal", False), **kw)
    k_all, v_all = (k4, v4) if not past else (np.concatenate([pk, k4], 2), np.concatenate([pv, v4], 2))
    assert np.array_equal(present_k, k_all) and np.array_equal(present_v, v_all)
    want = A.naive(q4, k_all, v_all, mask, past, case.get("nonpad"), case.get("causal", False), float(F(1.0) / np.sqrt(F(d))))
    out4 = out if rank == 4 else out.reshape(b, sq, hq, dv).transpose(0, 2, 1, 3)
    expect_equal(out4, want, str(case))
    if mask is not None and mask.dtype == I:
        assert not out4[:, 1].any()  # the fully masked rows are zeros, not NaN


z = lambda *shape: np.zeros(shape, F)
ERRORS = [
    ("InvalidValue", "query must have 3 or 4 dimensions", lambda: ([z(2, 8), z(2, 8), z(2, 8)], {})),
    ("IncompatibleInputShapes", "query, key and value must have the same rank", lambda: ([z(1, 2, 8), z(1, 1, 2, 8), z(1, 2, 8)], {})),
    ("InvalidValue", "q_num_heads is required for 3D inputs", lambda: ([z(1, 2, 8)] * 3, dict(kv_num_heads=1))),
    ("InvalidValue", "kv_num_heads is required for 3D inputs", lambda: ([z(1, 2, 8)] * 3, dict(q_num_heads=1))),
    ("InvalidValue", "q_num_heads and kv_num_heads must be positive", lambda: ([z(1, 2, 8)] * 3, dict(q_num_heads=0, kv_num_heads=1))),
    ("IncompatibleInputShapes", "query, key and value must have the same batch size", lambda: ([z(1, 2, 8), z(2, 2, 8), z(2, 2, 8)], dict(q_num_heads=1, kv_num_heads=1))),
    ("IncompatibleInputShapes", "key and value must have the same sequence length", lambda: ([z(1, 2, 8), z(1, 2, 8), z(1, 3, 8)], dict(q_num_heads=1, kv_num_heads=1))),
    ("IncompatibleInputShapes", "query hidden size must be divisible by q_num_heads", lambda: ([z(1, 2, 8)] * 3, dict(q_num_heads=3, kv_num_heads=1))),
    ("IncompatibleInputShapes", "key/value hidden size must be divisible by kv_num_heads", lambda: ([z(1, 2, 8), z(1, 2, 9), z(1, 2, 8)], dict(q_num_heads=2, kv_num_heads=2))),
    ("IncompatibleInputShapes", "key head size must match query head size", lambda: ([z(1, 2, 8), z(1, 2, 16), z(1, 2, 8)], dict(q_num_heads=2, kv_num_heads=2))),
    ("IncompatibleInputShapes", "key and value must have the same number of heads and sequence length", lambda: ([z(1, 2, 2, 8), z(1, 2, 2, 8), z(1, 1, 2, 8)], {})),
    ("IncompatibleInputShapes", "key head size must match query head size", lambda: ([z(1, 2, 2, 8), z(1, 2, 2, 4), z(1, 2, 2, 4)], {})),
    ("IncompatibleInputShapes", "q_num_heads must be a positive multiple of kv_num_heads", lambda: ([z(1, 3, 2, 8), z(1, 2, 2, 8), z(1, 2, 2, 8)], {})),
    ("IncompatibleInputShapes", "past_key/past_value shape does not match key/value shape", lambda: ([z(1, 2, 1, 8)] * 3 + [None, z(1, 2, 3, 8), z(1, 2, 4, 8)], {})),
    ("InvalidValue", "past_key and past_value must either both be present or both be absent", lambda: ([z(1, 2, 1, 8)] * 3 + [None, z(1, 2, 3, 8), None], {})),
    ("InvalidValue", "nonpad_kv_seqlen cannot be combined with past_key/past_value",
     lambda: ([z(1, 2, 1, 8)] * 3 + [None, z(1, 2, 3, 8), z(1, 2, 3, 8), np.array([1], I)], {})),
    ("IncompatibleInputShapes", "nonpad_kv_seqlen must have batch_size elements", lambda: ([z(1, 2, 1, 8)] * 3 + [None, None, None, np.array([1, 1], I)], {})),
    ("InvalidValue", "nonpad_kv_seqlen entry is out of range", lambda: ([z(1, 2, 1, 8)] * 3 + [None, None, None, np.array([2], I)], {})),
    ("IncompatibleInputShapes", "Cannot broadcast inputs", lambda: ([z(1, 2, 1, 8)] * 3 + [z(1, 2, 1, 3)], {})),
    ("InvalidValue", "attn_mask must have a float or bool (int32) type", lambda: ([z(1, 2, 1, 8)] * 3 + [np.zeros((1, 1, 1, 1), np.int64)], {})),
    ("UnsupportedValue", "qk_matmul_output output is not supported", lambda: ([z(1, 2, 1, 8)] * 3, dict(outputs=(0, 3)))),
    ("UnsupportedValue", "softcap is not supported", lambda: ([z(1, 2, 1, 8)] * 3, dict(softcap=30.0))),
]


@pytest.mark.parametrize("kind,msg,build", ERRORS, ids=[f"{i}-{e[1][:40]}" for i, e in enumerate(ERRORS)])
def test_rule_and_python_operator_refuse_with_the_reference_s_strings(kind, msg, build):
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    inputs, attrs = build()
    outputs = attrs.pop("outputs", (0, 1, 2))
    with pytest.raises(A.OpError) as e:
        A.attention(*inputs, **attrs, outputs=outputs)
    assert (e.value.kind, e.value.msg) == (kind, msg)
    ctx = _recording()
    dev = lambda i, a: a if a is None or i == 6 else DeviceTensor(ctx, a.shape, a.dtype)  # (nonpad_kv_seqlen stays a host value: validated)
    with pytest.raises(ops.OpError) as e:
        ops.Attention(**attrs).run(ctx, [dev(i, a) for i, a in enumerate(inputs)], outputs=outputs)
    assert (e.value.kind, e.value.msg) == (kind, msg)
    assert not [n for n, _ in ctx.calls if n.startswith("rten_hip_attention")]


def test_loader_parses_attention_graph_and_refuses_by_node_name(tmp_path):
    from rten_amd import onnx_writer as ow
    from tests.test_graph_executor import run_cli

    def parse(data):
        p = tmp_path / "m.onnx"
        p.write_bytes(data)
        return run_cli("--parse-only", str(p))

    for kw, words in ((dict(), "q_num_heads 8, kv_num_heads 2, not causal, present caches read"),
                      (dict(rank=4, mask=ow.INT32, past=False, nonpad=True, is_causal=1), "q_num_heads from the shape, kv_num_heads from the shape, causal")):
        r = parse(ow.attention_graph(**kw))
        assert r.returncode == 0 and 'attention step Attention "attention": ' + words in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    for kw, words in ((dict(softcap=30.0), "softcap != 0 is not supported"), (dict(qk_matmul_output_mode=1), "the qk_matmul_output_mode attribute is not supported"),
                      (dict(softmax_precision=1), "the softmax_precision attribute is not supported"), (dict(qk_output=True), "output 3 (qk_matmul_output, \"qk\") is read"),
                      (dict(input_type=ow.INT32), "input 0 (\"q\") has element type 6: float32 only"), (dict(mask=ow.INT64), "input 3 (\"attn_mask\") has element type 7")):
        r = parse(ow.attention_graph(**kw))
        assert r.returncode == 1 and "Attention attention: " + words in r.stderr, (kw, r.stdout[-1500:] + r.stderr[-1500:])
