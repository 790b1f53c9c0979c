"""Expected values for com.microsoft.GroupQueryAttention with a KV cache, restated on the oracle (the expectations of tests/test_gqa_ops.py and
tests/test_gpu_gqa.py).  Written from the reference (src/ops/attention/contrib.rs:359-878, sdpa_head at src/ops/attention.rs:518-562, the attribute
reader at src/op_registry/onnx_registry.rs:1467-1492), not from the device code.

  * scores = ref.gemm_f32(alpha = scale) on a transposed VIEW of the K slice: the oracle honours strides and takes the reference's vector-matrix kernels
    for one query row (unit row stride of B: the transposed form), the blocked order otherwise.
  * the score modification is numpy: the bias is added inside the window, every other position is overwritten with -inf.
  * ref.softmax(flush_nan = True), then ref.gemm_f32 for the second product.
  * rotary is decoder_rules.rotary_embedding on the [B, H, S, D] permutation, with position_ids or past_len + s.
  * the present cache is zero-filled; rows of `past` at or beyond past_len are dropped.
Errors carry the reference's kind and string (OpError below compares like rten_amd.ops.OpError).
"""
import numpy as np

from oracle import ref
from tests import decoder_rules

F = np.float32


class OpError(Exception):
    def __init__(self, kind, msg=""):
        super().__init__(f"{kind}({msg!r})")
        self.kind, self.msg = kind, msg

    def __eq__(self, other):
        return (self.kind, self.msg) == (getattr(other, "kind", None), getattr(other, "msg", None))

    __hash__ = Exception.__hash__


def read_attrs(attrs):
    """onnx_registry.rs:1467-1492 -> keyword arguments of group_query_attention."""
    if "num_heads" not in attrs or "kv_num_heads" not in attrs:
        raise OpError("MissingAttr", "num_heads" if "num_heads" not in attrs else "kv_num_heads")
    lw = attrs.get("local_window_size")
    return dict(num_heads=int(attrs["num_heads"]), kv_num_heads=int(attrs["kv_num_heads"]), scale=attrs.get("scale"),
                do_rotary=bool(attrs.get("do_rotary", 0)), rotary_interleaved=bool(attrs.get("rotary_interleaved", 0)),
                local_window_size=lw if lw is not None and lw > 0 else None, softcap=float(attrs.get("softcap", 0.0)),
                smooth_softmax=bool(attrs.get("smooth_softmax", 0)))


def present_cache(past, new, past_len, present_seq):
    """gqa_present_cache (contrib.rs:369-417): new is [B, S, KV, D], past [B, KV, P, D] or None."""
    batch, seq, kv_heads, head_size = new.shape
    present = np.zeros((batch, kv_heads, present_seq, head_size), F)
    for b in range(batch):
        pl = past_len(b)
        for h in range(kv_heads):
            if past is not None:
                present[b, h, :pl] = past[b, h, :pl]
            present[b, h, pl:pl + seq] = new[b, :, h]
    return present


def group_query_attention(query, key, value, past_key, past_value, seqlens_k, total_sequence_length, cos_cache=None, sin_cache=None, position_ids=None,
                          attention_bias=None, head_sink=None, *, num_heads, kv_num_heads, scale=None, do_rotary=False, rotary_interleaved=False,
                          local_window_size=None, softcap=0.0, smooth_softmax=False, outputs=(0, 1, 2)):
    """GroupQueryAttention::run_impl (contrib.rs:438-810) -> [output] or [output, present_key, present_value]."""
    query = np.asarray(query, F)
    if query.ndim != 3:
        raise OpError("InputCastFailed", "expected tensor with 3 dims")
    seqlens_k = np.asarray(seqlens_k, np.int32)
    while seqlens_k.ndim > 1 and seqlens_k.shape[-1] == 1:
        seqlens_k = seqlens_k.reshape(seqlens_k.shape[:-1])
    if seqlens_k.ndim != 1:
        raise OpError("UnsupportedValue", "seqlens_k must be a vector")
    if head_sink is not None:
        raise OpError("UnsupportedValue", "head_sink is not supported")
    if smooth_softmax:
        raise OpError("UnsupportedValue", "smooth_softmax is not supported")
    if num_heads == 0 or kv_num_heads == 0:
        raise OpError("InvalidValue", "num_heads and kv_num_heads must be positive")
    if num_heads % kv_num_heads != 0:
        raise OpError("InvalidValue", "num_heads must be a multiple of kv_num_heads")
    batch, seq, q_hidden = query.shape
    if key is not None and value is not None:
        key, value = np.asarray(key, F), np.asarray(value, F)
        if q_hidden % num_heads != 0:
            raise OpError("IncompatibleInputShapes", "query hidden size must be divisible by num_heads")
        head_size = q_hidden // num_heads
        if key.shape[0] != batch or value.shape[0] != batch:
            raise OpError("IncompatibleInputShapes", "key and value batch size must match query")
        if key.shape[1] != value.shape[1] or key.shape[2] != value.shape[2]:
            raise OpError("IncompatibleInputShapes", "key and value must have the same shape")
        if key.shape[2] != kv_num_heads * head_size:
            raise OpError("IncompatibleInputShapes", "key hidden size must equal kv_num_heads * head_size")
        if key.shape[1] != seq:
            raise OpError("UnsupportedValue", "key sequence length must match query sequence length")
        q4 = query.reshape(batch, seq, num_heads, head_size)
        k4 = key.reshape(batch, seq, kv_num_heads, head_size)
        v4 = value.reshape(batch, seq, kv_num_heads, head_size)
    elif key is None and value is None:
        total_heads = num_heads + 2 * kv_num_heads
        if q_hidden % total_heads != 0:
            raise OpError("IncompatibleInputShapes", "packed query hidden size must be divisible by num_heads + 2 * kv_num_heads")
        head_size = q_hidden // total_heads
        packed = query.reshape(batch, seq, total_heads, head_size)
        q4, k4, v4 = packed[:, :, :num_heads], packed[:, :, num_heads:num_heads + kv_num_heads], packed[:, :, num_heads + kv_num_heads:]
    else:
        raise OpError("InvalidValue", "key and value must both be present or both absent")
    if seqlens_k.shape[0] != batch:
        raise OpError("IncompatibleInputShapes", "seqlens_k must have batch_size elements")
    total = int(np.asarray(total_sequence_length).reshape(()))
    if total <= 0:
        raise OpError("InvalidValue", "total_sequence_length must be positive")
    if past_key is not None and past_value is not None:
        past_key, past_value = np.asarray(past_key, F), np.asarray(past_value, F)
        if past_key.shape != past_value.shape or past_key.shape[:2] != (batch, kv_num_heads) or past_key.shape[3] != head_size:
            raise OpError("IncompatibleInputShapes", "past_key/past_value shape does not match")
        past_seq = past_key.shape[2]
    elif past_key is None and past_value is None:
        past_seq = 0
    else:
        raise OpError("InvalidValue", "past_key and past_value must both be present or both absent")
    present_seq = past_seq + seq
    first, subsequent = seq == total, seq > 1 and seq != total
    if subsequent and batch != 1:
        raise OpError("UnsupportedValue", "batch size must be 1 when sequence_length > 1 and a past context is given")
    if not first and not subsequent and seq != 1:
        raise OpError("InvalidValue", "sequence_length must be 1 when query is not a prompt")
    for n in seqlens_k:
        if n < 0 or n >= present_seq:
            raise OpError("InvalidValue", "seqlens_k entry is out of range")
        if n + 1 < seq:
            raise OpError("InvalidValue", "seqlens_k entry is too small for the query sequence length")
    if attention_bias is not None:
        attention_bias = np.ascontiguousarray(attention_bias, F)
        bb, bh, bs, bt = attention_bias.shape
        if (bb != 1 and bb != batch) or (bh != 1 and bh != num_heads) or bs < seq or bt < present_seq:
            raise OpError("IncompatibleInputShapes", "attention_bias shape is incompatible with query/key shapes")

    def past_len(b):
        return 0 if first else int(seqlens_k[b]) + 1 - seq

    if scale is None:
        scale = float(F(1.0) / np.sqrt(F(head_size)))
    if do_rotary:
        if cos_cache is None or sin_cache is None:
            raise OpError("InvalidValue", "cos_cache and sin_cache are required when do_rotary is set")
        cos_cache, sin_cache = np.asarray(cos_cache, F), np.asarray(sin_cache, F)
        rotary_dim = cos_cache.shape[1] * 2
        if position_ids is not None:
            pos = np.asarray(position_ids, np.int32)
        else:
            pos = np.array([[past_len(b) + s for s in range(seq)] for b in range(batch)], np.int32).reshape(batch, seq)
        try:
            q4 = decoder_rules.rotary_embedding(q4.transpose(0, 2, 1, 3), cos_cache, sin_cache, pos, rotary_interleaved, num_heads, rotary_dim).transpose(0, 2, 1, 3)
            k4 = decoder_rules.rotary_embedding(k4.transpose(0, 2, 1, 3), cos_cache, sin_cache, pos, rotary_interleaved, kv_num_heads, rotary_dim).transpose(0, 2, 1, 3)
        except decoder_rules.RuleError as e:
            raise OpError(e.kind, e.msg)
    present_key = present_cache(past_key, k4, past_len, present_seq)
    present_value = present_cache(past_value, v4, past_len, present_seq)
    if softcap != 0.0:
        raise OpError("UnsupportedValue", "softcap is not restated (the reference calls libm's tanh)")

    kv_factor = num_heads // kv_num_heads
    out = np.empty((batch, num_heads, seq, head_size), F)
    for b in range(batch):
        kv_len = int(seqlens_k[b]) + 1
        for h in range(num_heads):
            g = h // kv_factor
            q_head = np.ascontiguousarray(q4[b, :, h])
            k_head, v_head = present_key[b, g, :kv_len], present_value[b, g, :kv_len]
            with np.errstate(all="ignore"):
                scores = ref.gemm_f32(q_head, k_head.T, alpha=scale)  # a transposed view: nothing is copied
                for s in range(seq):
                    lim = past_len(b) + s + 1
                    start = lim - local_window_size if local_window_size is not None and lim > local_window_size else 0
                    if attention_bias is not None:
                        bias = attention_bias[0 if attention_bias.shape[0] == 1 else b, 0 if attention_bias.shape[1] == 1 else h, s]
                        scores[s, start:lim] = scores[s, start:lim] + bias[start:lim]
                    scores[s, :start] = -np.inf
                    scores[s, lim:] = -np.inf
                probs = ref.softmax(scores, flush_nan=True)
                out[b, h] = ref.gemm_f32(probs, v_head)
    output = np.ascontiguousarray(out.transpose(0, 2, 1, 3)).reshape(batch, seq, num_heads * head_size)
    if 1 in outputs or 2 in outputs:
        return [output, present_key, present_value]
    return [output]


def naive(query, key, value, past_key, past_value, num_heads, kv_num_heads, scale):
    """reference_gqa of the reference's tests (contrib.rs:899-958): k-ordered float32 sums, softmax on the oracle's exp order (SoftmaxSimd)."""
    batch, seq, q_hidden = query.shape
    head_size = q_hidden // num_heads
    past_seq = 0 if past_key is None else past_key.shape[2]
    total = past_seq + seq
    kf = num_heads // kv_num_heads

    def gather(new, past):
        full = np.empty((batch, kv_num_heads, total, head_size), F)
        if past is not None:
            full[:, :, :past_seq] = past
        full[:, :, past_seq:] = new.reshape(batch, seq, kv_num_heads, head_size).transpose(0, 2, 1, 3)
        return full

    k_full, v_full = gather(key, past_key), gather(value, past_value)
    out = np.zeros((batch, seq, q_hidden), F)
    for b in range(batch):
        for n in range(num_heads):
            g = n // kf
            for s in range(seq):
                limit = past_seq + s + 1
                scores = np.empty(limit, F)
                for t in range(limit):
                    dot = F(0)
                    for d in range(head_size):
                        dot = F(dot + F(query[b, s, n * head_size + d] * k_full[b, g, t, d]))
                    scores[t] = F(dot * F(scale))
                probs = ref.softmax(scores.reshape(1, -1)).reshape(-1)
                for d in range(head_size):
                    acc = F(0)
                    for t in range(limit):
                        acc = F(acc + F(probs[t] * v_full[b, g, t, d]))
                    out[b, s, n * head_size + d] = acc
    return out


def clamped_lengths(seqlens_k, total, seq, past_seq):
    """What the device does with values it alone knows (docs/KERNELS.md deviation table): kv_len into [1, P + S], past_len into [0, P]."""
    kv = np.clip(np.asarray(seqlens_k, np.int64) + 1, 1, past_seq + seq)
    pl = np.zeros_like(kv) if int(total) == seq else np.clip(kv - seq, 0, past_seq)
    return kv, pl
