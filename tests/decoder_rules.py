"""Expected values for RMSNormalization / SimplifiedLayerNormalization, SkipLayerNormalization / SkipSimplifiedLayerNormalization and the two RotaryEmbedding
operators, restated in numpy float32 (the expectations of tests/test_decoder_ops.py and tests/test_gpu_decoder.py).  Written from the reference
(src/ops/norm.rs:103-161,419-529,571-608, src/ops/norm/contrib.rs:22-238, rten-vecmath/src/normalize.rs:112-166, src/ops/embedding.rs:20-207,
src/ops/embedding/contrib.rs:32-126, src/ops/gather.rs), not from the device code.

  * SumSquare is reduce_rules.sum_square: fold_unroll<4> over 16-lane vectors with acc = fmaf(x, x, acc), lanes added from lane 0.
  * r = scale / sqrt(ms + eps): numpy's float32 sqrt and division are correctly rounded, as Rust's are.
  * The element map is one of Normalize's arms: a one-element scale gives mul_add(x - 0, r, 0) (libm's fmaf: a -0 product comes out +0), a per-element one
    (x - 0) * (scale[i] * r).
  * The LayerNorm mode of the skip form is the oracle's layer_norm (oracle.ref) of the sum.
  * Rotary: every product and the sum or difference are rounded on their own (Rust does not contract).
"""
import numpy as np

from oracle import ref
from tests import reduce_rules
from tests.reduce_rules import RuleError, fmaf

F = np.float32


def _resolve_axis(nd, axis):
    if axis < -nd or axis >= nd:
        raise RuleError("InvalidValue", "Axis is invalid")
    return axis + nd if axis < 0 else axis


def _item(t):
    t = np.asarray(t)
    return t.reshape(()) if t.size == 1 else None


def rms_row(x, scale, scale_scalar, eps):
    """normalize_slice with MeanNormalize::DynamicRootMeanSquare (norm.rs:128-160): scale = per-element array or None."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        ms = F(reduce_rules.sum_square(x) / F(x.size))
        r = F(F(scale_scalar) / np.sqrt(F(ms + F(eps))))
        y0 = (x - F(0)).astype(np.float32)
        if scale is None:
            return np.array([fmaf(v, r, F(0)) for v in y0], np.float32)
        return (y0 * (np.asarray(scale, np.float32) * r).astype(np.float32)).astype(np.float32)


def rms_normalization(x, scale, axis=-1, epsilon=None):
    """rms_normalization -> layer_normalization_impl (norm.rs:419-529)."""
    x, scale = np.asarray(x, np.float32), np.asarray(scale, np.float32)
    eps = 1e-5 if epsilon is None else epsilon
    ax = _resolve_axis(x.ndim, axis)
    norm_shape = x.shape[ax:]
    it = _item(scale)
    if it is None:
        try:
            elems = np.ascontiguousarray(np.broadcast_to(scale, norm_shape)).reshape(-1)
        except ValueError:
            raise RuleError("InvalidValue", "`scale` is not broadcastable to normalized axes of input")
    cols = int(np.prod(norm_shape, dtype=np.int64))
    rows = np.ascontiguousarray(x).reshape(-1, cols) if x.size else np.zeros((0, cols), np.float32)
    y = np.empty_like(rows)
    for i in range(rows.shape[0]):
        y[i] = rms_row(rows[i], None if it is not None else elems, it if it is not None else 1.0, eps)
    return y.reshape(x.shape)


def layer_normalization_last(x, gamma, beta, epsilon):
    """layer_normalization_impl with MeanNormalize::Dynamic over the last axis, gamma [H], beta [H] or None: the oracle's LayerNormalization."""
    g, b = np.asarray(gamma, np.float32), None if beta is None else np.asarray(beta, np.float32)
    kw = {}
    if g.size == 1:
        kw["gamma_scalar"], g = float(g.reshape(())), None
    if b is not None and b.size == 1:
        kw["beta_scalar"], b = float(b.reshape(())), None
    return ref.layer_norm(np.asarray(x, np.float32), g, b, eps=epsilon, **kw)


def skip_norm(x, skip, gamma, beta=None, bias=None, epsilon=1e-5, rms=False):
    """skip_layer_normalization (contrib.rs:22-77): returns (output, input_skip_bias_sum)."""
    x, skip = np.asarray(x, np.float32), np.asarray(skip, np.float32)
    if x.ndim not in (2, 3):
        raise RuleError("InvalidValue", "input must be 2 or 3 dimensioned")
    if skip.ndim not in (2, 3):
        raise RuleError("InvalidValue", "skip must be 2 or 3 dimensioned")
    can = skip.ndim <= x.ndim and all(s in (1, d) for s, d in zip(skip.shape[::-1], x.shape[::-1]))
    if skip.shape[-2:] != x.shape[-2:] or not can:
        raise RuleError("IncompatibleInputShapes", "skip must broadcast to input over the batch dimension")
    with np.errstate(all="ignore"):
        total = (x + skip).astype(np.float32)
        if bias is not None:
            total = (total + np.asarray(bias, np.float32)).astype(np.float32)
    y = rms_normalization(total, gamma, -1, epsilon) if rms else layer_normalization_last(total, gamma, beta, epsilon)
    return y, total


def rotary_cache_dims(cache_shape, batch, seq_len, half, bad_last_dim):
    """embedding.rs:20-44."""
    if len(cache_shape) != 3:
        raise RuleError("InvalidValue", "cos/sin cache must be a 3D tensor")
    cb, cs, ch = cache_shape
    if ch != half:
        raise RuleError("InvalidValue", bad_last_dim)
    if cs != 1 and cs != seq_len:
        raise RuleError("InvalidValue", "cos/sin cache sequence length must be 1 or match the input")
    if cb != 1 and cb != batch:
        raise RuleError("InvalidValue", "cos/sin cache batch size must be 1 or match the input")
    return cb, cs


def gather0(table, ids):
    """gather along axis 0 (gather.rs): a negative index counts from the end; one outside [-len, len) is an error."""
    table, ids = np.asarray(table), np.asarray(ids)
    n = table.shape[0]
    if ids.size and (ids.min() < -n or ids.max() >= n):
        raise RuleError("InvalidValue", "Entry in `indices` is out of range")
    return table[np.where(ids < 0, ids + n, ids)]


def clamp_ids(ids, n):
    """What the device does with an id it alone knows (KERNELS.md deviation table, Gather): a negative id counts from the end, then into [0, n)."""
    ids = np.asarray(ids, np.int64)
    return np.clip(np.where(ids < 0, ids + n, ids), 0, n - 1)


def rotary_embedding(x, cos, sin, position_ids=None, interleaved=False, num_heads=0, rotary_embedding_dim=0):
    """rotary_embedding (embedding.rs:46-207)."""
    x, cos, sin = np.asarray(x, np.float32), np.asarray(cos, np.float32), np.asarray(sin, np.float32)
    if x.ndim == 3:
        batch, seq_len, hidden = x.shape
        if num_heads == 0:
            raise RuleError("InvalidValue", "num_heads must not be 0 for 3 dimensioned input")
        if hidden % num_heads != 0:
            raise RuleError("InvalidValue", "hidden_size must be divisible by num_heads")
        xr = x.reshape(batch, seq_len, num_heads, hidden // num_heads)
    elif x.ndim == 4:
        xr = x.transpose(0, 2, 1, 3)
    else:
        raise RuleError("IncompatibleInputShapes", "Input processed needs 3-4 dimensions")
    batch, seq_len, heads, head_size = xr.shape
    rot = head_size if rotary_embedding_dim == 0 else rotary_embedding_dim
    if rot == 0 or rot % 2 != 0:
        raise RuleError("InvalidValue", "rotary_embedding_dim must be a positive even number")
    if rot > head_size:
        raise RuleError("InvalidValue", "rotary_embedding_dim must not exceed head size")
    half = rot // 2
    if position_ids is not None:
        cos, sin = gather0(cos, position_ids), gather0(sin, position_ids)
    cb, cs = rotary_cache_dims(cos.shape, batch, seq_len, half, "Last dimension of cos cache does not match rotary_embedding_dim/2")
    sb, ss = rotary_cache_dims(sin.shape, batch, seq_len, half, "Last dimension of sin cache does not match rotary_embedding_dim/2")
    c = np.broadcast_to(cos, (batch, seq_len, half))[:, :, None, :]
    s = np.broadcast_to(sin, (batch, seq_len, half))[:, :, None, :]
    y = xr.copy()
    if interleaved:
        x1, x2 = xr[..., 0:rot:2], xr[..., 1:rot:2]
    else:
        x1, x2 = xr[..., :half], xr[..., half:rot]
    with np.errstate(all="ignore"):
        y1 = ((x1 * c).astype(np.float32) - (x2 * s).astype(np.float32)).astype(np.float32)
        y2 = ((x1 * s).astype(np.float32) + (x2 * c).astype(np.float32)).astype(np.float32)
    if interleaved:
        y[..., 0:rot:2], y[..., 1:rot:2] = y1, y2
    else:
        y[..., :half], y[..., half:rot] = y1, y2
    return np.ascontiguousarray(y.reshape(x.shape) if x.ndim == 3 else y.transpose(0, 2, 1, 3))


def rotary_embedding_microsoft(x, position_ids, cos, sin, interleaved=False, num_heads=None, rotary_embedding_dim=0):
    """RotaryEmbeddingMicrosoft::run (embedding/contrib.rs:32-126)."""
    x, ids, cos = np.asarray(x, np.float32), np.asarray(position_ids), np.asarray(cos, np.float32)
    if x.ndim == 3:
        batch, seq_len = x.shape[0], x.shape[1]
    elif x.ndim == 4:
        batch, seq_len = x.shape[0], x.shape[2]
    else:
        raise RuleError("IncompatibleInputShapes", "Input processed needs 3-4 dimensions")
    if ids.ndim in (0, 1) and ids.size == 1:
        ids = (int(ids.reshape(())) + np.arange(seq_len, dtype=np.int64))[None, :].repeat(batch, axis=0)
    elif ids.ndim != 2:
        raise RuleError("InvalidValue", "position_ids must be a scalar, a 1-element vector or have 2 dims")
    heads = num_heads or 0
    if x.ndim == 3 and heads == 0:
        if rotary_embedding_dim != 0:
            raise RuleError("InvalidValue", "num_heads must be specified when rotary_embedding_dim is set")
        if cos.ndim == 0:
            raise RuleError("InvalidValue", "cos cache must not be scalar")
        if cos.shape[-1] == 0:
            raise RuleError("InvalidValue", "Last dimension of cos cache must not be 0")
        if x.shape[2] % (cos.shape[-1] * 2) != 0:
            raise RuleError("InvalidValue", "hidden_size must be divisible by head size")
        heads = x.shape[2] // (cos.shape[-1] * 2)
    return rotary_embedding(x, cos, sin, ids, interleaved, heads, rotary_embedding_dim)


def silu(x):
    """The gated MLP's activation as tests/norm_rules.py restates it: x / (1 + exp(-x)) on the oracle's exp."""
    from rten_amd import lib as L
    from tests import norm_rules
    return norm_rules.activation(L.ACT_SILU, x)
