"""Expected values for the opset-23 Attention operator with past / present caches, restated on the oracle (the expectations of tests/test_attention_ops.py
and tests/test_gpu_attention.py).  Written from the reference (Attention::run_impl, src/ops/attention.rs:579-973, on sdpa_head :518-562 and concat_past_kv
:470-507; attributes onnx_registry.rs:791-810), not from the device code.

  * 3-D inputs become (B, H, S, D) VIEWS (split_attention_heads); present is concat(past, current) on axis 2, or the current K / V.
  * scores = ref.gemm_f32(alpha = scale) on a transposed view of the K slice, over all T = past_seq + kv_seq columns: nothing stops at nonpad.
  * per row: float mask added / bool mask overwrites with -inf, then the causal fill from clamp(offset + q_idx + 1, 0, T), or else the nonpad fill.
  * ref.softmax(flush_nan = True), then ref.gemm_f32 for the second product.
softcap > 0 is refused: the reference calls libm's tanh there, which is not the restated vecmath tanh (tests/gqa_rules.py refuses it for the same reason).
"""
import numpy as np

from oracle import ref
from tests.gqa_rules import OpError

F = np.float32
BROADCAST = "Cannot broadcast inputs"


def attention(query, key, value, attn_mask=None, past_key=None, past_value=None, nonpad_kv_seqlen=None, *, is_causal=False, q_num_heads=None,
              kv_num_heads=None, scale=None, softcap=0.0, outputs=(0, 1, 2)):
    """-> [output] or [output, present_key, present_value] (present always 4-D)."""
    if 3 in outputs:
        raise OpError("UnsupportedValue", "qk_matmul_output output is not supported")
    query, key, value = np.asarray(query, F), np.asarray(key, F), np.asarray(value, F)
    if query.ndim not in (3, 4):
        raise OpError("InvalidValue", "query must have 3 or 4 dimensions")
    if key.ndim != query.ndim or value.ndim != query.ndim:
        raise OpError("IncompatibleInputShapes", "query, key and value must have the same rank")
    input_3d = query.ndim == 3
    if input_3d:
        if q_num_heads is None:
            raise OpError("InvalidValue", "q_num_heads is required for 3D inputs")
        if kv_num_heads is None:
            raise OpError("InvalidValue", "kv_num_heads is required for 3D inputs")
        if q_num_heads == 0 or kv_num_heads == 0:
            raise OpError("InvalidValue", "q_num_heads and kv_num_heads must be positive")
        batch, q_seq, q_hidden = query.shape
        if key.shape[0] != batch or value.shape[0] != batch:
            raise OpError("IncompatibleInputShapes", "query, key and value must have the same batch size")
        if key.shape[1] != value.shape[1]:
            raise OpError("IncompatibleInputShapes", "key and value must have the same sequence length")
        if q_hidden % q_num_heads != 0:
            raise OpError("IncompatibleInputShapes", "query hidden size must be divisible by q_num_heads")
        head_size = q_hidden // q_num_heads
        if key.shape[2] % kv_num_heads != 0 or value.shape[2] % kv_num_heads != 0:
            raise OpError("IncompatibleInputShapes", "key/value hidden size must be divisible by kv_num_heads")
        if key.shape[2] // kv_num_heads != head_size:
            raise OpError("IncompatibleInputShapes", "key head size must match query head size")
        split = lambda x, heads: x.reshape(x.shape[0], x.shape[1], heads, x.shape[2] // heads).transpose(0, 2, 1, 3)  # a view
        query, key, value = split(query, q_num_heads), split(key, kv_num_heads), split(value, kv_num_heads)
    else:
        batch = query.shape[0]
        if key.shape[0] != batch or value.shape[0] != batch:
            raise OpError("IncompatibleInputShapes", "query, key and value must have the same batch size")
        if key.shape[1] != value.shape[1] or key.shape[2] != value.shape[2]:
            raise OpError("IncompatibleInputShapes", "key and value must have the same number of heads and sequence length")
        if key.shape[3] != query.shape[3]:
            raise OpError("IncompatibleInputShapes", "key head size must match query head size")
    batch, q_heads, q_seq, head_size = query.shape
    kv_heads = key.shape[1]
    if q_heads == 0 or kv_heads == 0 or q_heads % kv_heads != 0:
        raise OpError("IncompatibleInputShapes", "q_num_heads must be a positive multiple of kv_num_heads")
    has_past = past_key is not None
    if past_key is not None and past_value is not None:
        past_key, past_value = np.asarray(past_key, F), np.asarray(past_value, F)
        if past_key.shape[:2] != (batch, kv_heads) or past_value.shape[:2] != (batch, kv_heads) or past_key.shape[3] != head_size or \
                past_value.shape[3] != value.shape[3] or past_key.shape[2] != past_value.shape[2]:
            raise OpError("IncompatibleInputShapes", "past_key/past_value shape does not match key/value shape")
        past_len = past_key.shape[2]
        key, value = np.concatenate([past_key, key], axis=2), np.concatenate([past_value, value], axis=2)
    elif past_key is None and past_value is None:
        past_len = 0
    else:
        raise OpError("InvalidValue", "past_key and past_value must either both be present or both be absent")
    total = key.shape[2]
    nonpad = None
    if nonpad_kv_seqlen is not None:
        nonpad = np.asarray(nonpad_kv_seqlen, np.int32)
        if has_past:
            raise OpError("InvalidValue", "nonpad_kv_seqlen cannot be combined with past_key/past_value")
        if nonpad.shape != (batch,):
            raise OpError("IncompatibleInputShapes", "nonpad_kv_seqlen must have batch_size elements")
        if any(n < 0 or n > total for n in nonpad):
            raise OpError("InvalidValue", "nonpad_kv_seqlen entry is out of range")
    if scale is None:
        scale = float(F(1.0) / np.sqrt(F(head_size)))
    mask = None
    if attn_mask is not None:
        attn_mask = np.asarray(attn_mask)
        if attn_mask.dtype not in (np.float32, np.int32):
            raise OpError("InvalidValue", "attn_mask must have a float or bool (int32) type")
        try:
            mask = np.broadcast_to(attn_mask, (batch, q_heads, q_seq, total))
        except ValueError:
            raise OpError("IncompatibleInputShapes", BROADCAST)
        if attn_mask.ndim > 4:
            raise OpError("IncompatibleInputShapes", BROADCAST)
    if softcap > 0.0:
        raise OpError("UnsupportedValue", "softcap is not supported")  # (the reference calls libm's tanh there: not restated)

    kv_factor = q_heads // kv_heads
    out = np.empty((batch, q_heads, q_seq, value.shape[3]), F)
    for b in range(batch):
        for h in range(q_heads):
            k_head, v_head = key[b, h // kv_factor], value[b, h // kv_factor]
            with np.errstate(all="ignore"):
                scores = ref.gemm_f32(query[b, h], k_head.T, alpha=scale)  # views: the oracle honours the strides
                for s in range(q_seq):
                    if mask is not None and mask.dtype == np.float32:
                        scores[s] = scores[s] + mask[b, h, s]
                    elif mask is not None:
                        scores[s, mask[b, h, s] == 0] = -np.inf
                    if is_causal:
                        offset = int(nonpad[b]) - q_seq if nonpad is not None else past_len
                        scores[s, min(max(offset + s + 1, 0), total):] = -np.inf
                    elif nonpad is not None:
                        scores[s, int(nonpad[b]):] = -np.inf
                probs = ref.softmax(scores, flush_nan=True)
                out[b, h] = ref.gemm_f32(probs, v_head)
    if input_3d:
        out = np.ascontiguousarray(out.transpose(0, 2, 1, 3)).reshape(batch, q_seq, -1)
    if 1 in outputs or 2 in outputs:
        return [out, np.ascontiguousarray(key), np.ascontiguousarray(value)]
    return [out]


def naive(query, key, value, mask, past_len, nonpad, is_causal, scale):
    """float64 attention on 4-D arrays whose K / V already hold the past: the plain reference the rule is held to (tests/test_attention_ops.py)."""
    batch, q_heads, q_seq, _ = query.shape
    total, rep = key.shape[2], q_heads // key.shape[1]
    k, v = np.repeat(key.astype(np.float64), rep, axis=1), np.repeat(value.astype(np.float64), rep, axis=1)
    scores = np.einsum("bhsd,bhtd->bhst", query.astype(np.float64), k) * scale
    if mask is not None:
        m = np.broadcast_to(mask, scores.shape)
        scores = scores + m if mask.dtype == np.float32 else np.where(m == 0, -np.inf, scores)
    t = np.arange(total)
    for b in range(batch):
        for s in range(q_seq):
            if is_causal:
                scores[b, :, s, t >= (nonpad[b] - q_seq if nonpad is not None else past_len) + s + 1] = -np.inf
            elif nonpad is not None:
                scores[b, :, s, t >= nonpad[b]] = -np.inf
    with np.errstate(all="ignore"):
        e = np.exp(scores - scores.max(axis=-1, keepdims=True))
        probs = np.nan_to_num(e / e.sum(axis=-1, keepdims=True), nan=0.0)
    return np.einsum("bhst,bhtd->bhsd", probs, v)
