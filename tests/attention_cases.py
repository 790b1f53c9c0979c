"""Cases for rten_hip_attention_f32 called with raw strides (tests/test_gpu_attention_confine.py), built and proven on the CPU first
(tests/test_attention_cases.py), as tests/confine.py does for the older kernels.  Plain numpy on tests/attention_rules.py; no GPU.

A `Case` holds the host buffers of one call, the element offset of q, k and v inside them, the 16 strides of the entry point, and the
dense (B, H, S, D) operands the buffers were filled from: `expected(case)` is attention_rules.attention on those dense operands, and
`gathered(case)` reads them back through the strides, so a layout that does not describe its own buffers fails on the CPU.

  * strided_layouts: what the header promises beyond the two layouts ops.Attention produces.  Every element of a buffer that no
    operand names is NaN: a kernel that reads it and lets it reach an output fails the bit comparison.
  * nonfinite_cases: NaN / Inf at stated places INSIDE the operands, with the set of (batch, query head) outputs and present rows that
    may differ from the finite run.  The CPU test proves each set exact on the rule.
  * range_bands: operands whose scores overflow, whose exponentials all vanish but one, whose probabilities or products are subnormal,
    or whose row is masked entirely; each with a predicate on the rule's result, so a band cannot turn into ordinary values unnoticed.
"""
import functools
import types

import numpy as np

from oracle import ref
from tests import attention_rules as A

F, I = np.float32, np.int32
TINY = float(np.finfo(F).tiny)
MASK_NONE, MASK_FLOAT, MASK_BOOL = 0, 1, 2  # RTEN_HIP_ATTN_MASK_*


def noise(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


# ------------------------------------------------------------------------------------------------ placing a dense tensor into a buffer
def bhsd(shape, row_pad=0, head_pad=0):
    """(batch, head, row) strides of a (B, H, S, D) tensor whose rows are `row_pad` and whose heads `head_pad` elements apart."""
    _, h, s, d = shape
    ss = d + row_pad
    sh = s * ss + head_pad
    return h * sh, sh, ss


def bshd(shape, row_pad=0, batch_pad=0):
    """(batch, head, row) strides of the (B, S, H * D) layout, with slack after each row and each batch item."""
    _, h, s, d = shape
    ss = h * d + row_pad
    return s * ss + batch_pad, d, ss


def span(shape, strides):
    return 1 + sum((n - 1) * st for n, st in zip(shape, tuple(strides) + (1,))) if all(shape) else 0


def index(shape, strides, unit=True):
    """Element offsets of a tensor of `shape`; unit: `strides` lacks the last axis, whose stride is 1."""
    idx = np.zeros((), np.int64)
    for n, st in zip(shape, tuple(strides) + ((1,) if unit else ())):
        idx = idx[..., None] + np.arange(n, dtype=np.int64) * int(st)
    return idx


def scatter(buf, off, t4, strides):
    buf[off + index(t4.shape, strides)] = t4


def gather(buf, off, shape, strides):
    return np.ascontiguousarray(buf[off + index(shape, strides)])


def placed(t4, strides):
    """A NaN-filled buffer of exactly the tensor's span holding `t4` -> (buffer, offset 0)."""
    buf = np.full(span(t4.shape, strides), np.nan, t4.dtype)
    scatter(buf, 0, t4, strides)
    return buf


def make(name, q, k, v, pk=None, pv=None, mask=None, nonpad=None, causal=False, scale=None, q_st=None, k_st=None, v_st=None, o_st=None, m_st=None,
         packed=False):
    """A Case from dense (B, H, S, D) operands.  *_st: (batch, head, row) strides, default dense (B, H, S, D); m_st: the mask's four strides (default: the
    dense strides of its own shape, 0 on axes of extent 1); packed: q, k, v are column blocks of ONE [B, S, (Hq + 2 Hkv) * D] buffer."""
    b, hq, sq, d = q.shape
    hkv, skv, dv = k.shape[1], k.shape[2], v.shape[3]
    past = 0 if pk is None else pk.shape[2]
    c = types.SimpleNamespace(name=name, b=b, hq=hq, hkv=hkv, sq=sq, skv=skv, past=past, t=past + skv, d=d, dv=dv, causal=causal, scale=scale, q=q, k=k, v=v,
                              pk=pk, pv=pv, mask=mask, nonpad=None if nonpad is None else np.asarray(nonpad, I))
    if packed:
        assert sq == skv and d == dv
        row = (hq + 2 * hkv) * d
        st = (sq * row, d, row)
        buf = np.full(b * sq * row, np.nan, F)
        c.where = {"q": ("qkv", 0), "k": ("qkv", hq * d), "v": ("qkv", (hq + hkv) * d)}
        for t4, nm in ((q, "q"), (k, "k"), (v, "v")):
            scatter(buf, c.where[nm][1], t4, st)
        c.bufs = {"qkv": buf}
        q_st = k_st = v_st = st
    else:
        q_st, k_st, v_st = q_st or bhsd(q.shape), k_st or bhsd(k.shape), v_st or bhsd(v.shape)
        c.bufs = {"q": placed(q, q_st), "k": placed(k, k_st), "v": placed(v, v_st)}
        c.where = {nm: (nm, 0) for nm in "qkv"}
    c.o_shape = (b, hq, sq, dv)
    o_st = o_st or bhsd(c.o_shape)
    c.o_span = span(c.o_shape, o_st)
    c.mask_kind, c.mask_buf, m4 = MASK_NONE, None, (0, 0, 0, 0)
    if mask is not None:
        assert mask.ndim == 4 and mask.dtype in (F, I)
        c.mask_kind = MASK_FLOAT if mask.dtype == F else MASK_BOOL
        if m_st is None:
            dense, acc = [], 1
            for n in reversed(mask.shape):
                dense.append(0 if n == 1 else acc)
                acc *= n
            m_st = tuple(reversed(dense))
        m4 = tuple(0 if n == 1 else st for n, st in zip(mask.shape, m_st))
        # (a float mask's gaps are NaN, a bool mask's 0 = "masked": either changes the result when it is read)
        c.mask_buf = np.full(1 + sum((n - 1) * st for n, st in zip(mask.shape, m4)), np.nan if mask.dtype == F else 0, mask.dtype)
        c.mask_buf[index(mask.shape, m4, unit=False)] = mask
    c.strides = [*q_st, *k_st, *v_st, *o_st, *m4]
    return c


def gathered(c):
    """q, k, v and the mask read back out of the buffers through the case's strides."""
    st = c.strides
    q = gather(c.bufs[c.where["q"][0]], c.where["q"][1], (c.b, c.hq, c.sq, c.d), st[0:3])
    k = gather(c.bufs[c.where["k"][0]], c.where["k"][1], (c.b, c.hkv, c.skv, c.d), st[3:6])
    v = gather(c.bufs[c.where["v"][0]], c.where["v"][1], (c.b, c.hkv, c.skv, c.dv), st[6:9])
    mask = None
    if c.mask is not None:
        mask = c.mask_buf[index(c.mask.shape, st[12:16], unit=False)]
    return q, k, v, mask


def expected(c):
    """[out (B, Hq, Sq, Dv), present_key, present_value] by the rule, on the dense operands."""
    return A.attention(c.q, c.k, c.v, c.mask, c.pk, c.pv, c.nonpad, is_causal=c.causal, scale=c.scale)


def dense_operands(seed, b, hq, hkv, sq, skv, past, d, dv=None):
    dv = d if dv is None else dv
    pk, pv = (noise(seed + 3, b, hkv, past, d), noise(seed + 4, b, hkv, past, dv)) if past else (None, None)
    return noise(seed, b, hq, sq, d), noise(seed + 1, b, hkv, skv, d), noise(seed + 2, b, hkv, skv, dv), pk, pv


def standard(name, seed, b, hq, hkv, sq, skv, past, d, dv=None, rank=4, **kw):
    """One of the two layouts ops.Attention produces: (B, H, S, D) or (B, S, H * D)."""
    q, k, v, pk, pv = dense_operands(seed, b, hq, hkv, sq, skv, past, d, dv)
    if rank == 3:
        kw = dict(q_st=bshd(q.shape), k_st=bshd(k.shape), v_st=bshd(v.shape), o_st=bshd((b, hq, sq, v.shape[3])), **kw)
    return make(name, q, k, v, pk, pv, **kw)


# ------------------------------------------------------------------------------------------------ layouts
def strided_layouts(b, hq, hkv, sq, skv, d, dv, past=0, causal=False, seed=700):
    """Yields the named layouts the header promises and no operator produces."""
    q, k, v, pk, pv = dense_operands(seed, b, hq, hkv, sq, skv, past, d, dv)
    t = past + skv
    o_shape = (b, hq, sq, dv)
    if sq == skv and d == dv:
        yield make("packed-qkv", q, k, v, pk, pv, causal=causal, packed=True, o_st=bshd(o_shape))
    yield make("out-slack", q, k, v, pk, pv, causal=causal, q_st=bshd(q.shape), k_st=bshd(k.shape), v_st=bshd(v.shape), o_st=bshd(o_shape, 24, 40))
    yield make("bhsd-padded", q, k, v, pk, pv, causal=causal, k_st=bhsd(k.shape, 8, 16), v_st=bhsd(v.shape, 8, 16))
    fmask = noise(seed + 9, 1, hq, sq, t)
    bmask = (noise(seed + 10, 1, hq, sq, t) > -0.5).astype(I)
    bmask[..., 0] = 1  # (no fully masked row here: all_masked covers that)
    m_st = (0, sq * (t + 3) + 5, t + 3, 1)  # a real head stride and a real row stride at once, neither dense
    yield make("mask-head-and-row-float", q, k, v, pk, pv, causal=causal, mask=fmask, m_st=m_st)
    yield make("mask-head-and-row-bool", q, k, v, pk, pv, causal=causal, mask=bmask, m_st=m_st)


# ------------------------------------------------------------------------------------------------ non-finite values and what depends on them
NF = dict(b=2, hq=8, hkv=2, d=64, past=40)
NONFINITE = ("nan-k-row", "nan-masked-v-row", "inf-q-head", "nan-past-of-item-0")


@functools.lru_cache(maxsize=None)
def nonfinite_case(name):
    """-> (finite case, case with the non-finite values, dep) with dep = dict(out [B, Hq] bool, pk [B, Hkv, T] bool, pv [B, Hkv, T] bool): the (batch,
    query head) outputs and the present rows that may -- and on the rule do -- differ from the finite run."""
    b, hq, hkv, d, past = (NF[x] for x in ("b", "hq", "hkv", "d", "past"))
    g = hq // hkv
    if name == "nan-masked-v-row":  # nonpad is refused together with a past: an external cache of `past + 1` rows
        q, k, v, pk, pv = dense_operands(810, b, hq, hkv, 1, past + 1, 0, d)
        kw = dict(nonpad=[past + 1, 9])
    else:
        q, k, v, pk, pv = dense_operands(811, b, hq, hkv, 1, 1, past, d)
        kw = {}
    t = past + 1
    fin = make(name + " (finite)", q, k, v, pk, pv, **kw)
    q, k, v = q.copy(), k.copy(), v.copy()
    pk, pv = (None, None) if pk is None else (pk.copy(), pv.copy())
    dep = dict(out=np.zeros((b, hq), bool), pk=np.zeros((b, hkv, t), bool), pv=np.zeros((b, hkv, t), bool))
    if name == "nan-k-row":  # a visible key of (batch 1, KV head 0): that head's G query heads of batch 1, and that row of present_key
        pk[1, 0, 5] = np.nan
        dep["out"][1, 0:g] = True
        dep["pk"][1, 0, 5] = True
    elif name == "nan-masked-v-row":  # key 20 of KV head 1: visible for item 0, beyond nonpad for item 1 -- probability 0 times NaN propagates all the same
        v[:, 1, 20] = np.nan
        dep["out"][:, g:2 * g] = True
        dep["pv"][:, 1, 20] = True
    elif name == "inf-q-head":
        q[0, 3, 0, 7] = np.inf
        dep["out"][0, 3] = True
    elif name == "nan-past-of-item-0":
        pk[0, :, 3] = np.nan
        pv[0, :, 4] = np.nan
        dep["out"][0] = True
        dep["pk"][0, :, 3] = True
        dep["pv"][0, :, 4] = True
    else:
        raise KeyError(name)
    return fin, make(name, q, k, v, pk, pv, **kw), dep


def nonfinite_cases():
    return [nonfinite_case(n) for n in NONFINITE]


# ------------------------------------------------------------------------------------------------ operand range
BAND = dict(b=2, hq=8, hkv=2, d=64, t=135)
RANGE_BANDS = ("overflow_scores", "one_survivor", "subnormal_p", "all_masked")
SURVIVOR = 77  # the key that keeps all the probability in one_survivor


def wide(rng, shape, lo, hi):
    """Signed values whose magnitudes are 2^U(lo, hi)."""
    return (np.exp2(rng.uniform(lo, hi, shape)) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)).astype(F)


@functools.lru_cache(maxsize=None)
def range_band(name):
    """One query row on T = 135 keys (a past of 134 rows and one new row; all_masked: an external cache, since nonpad excludes a past)."""
    b, hq, hkv, d, t = (BAND[x] for x in ("b", "hq", "hkv", "d", "t"))
    g = hq // hkv
    rng = np.random.default_rng([ord(ch) for ch in name])
    kw = {}
    if name == "all_masked":
        q, k, v, pk, pv = dense_operands(901, b, hq, hkv, 1, t, 0, d)
        mask = noise(902, b, 1, 1, t)
        mask[0, 0, 0, 100:110] = -np.inf
        kw = dict(mask=mask, nonpad=[t, 0])  # item 1: every key is beyond nonpad -> the row is all -inf -> NaN -> flushed to 0
        return make(name, q, k, v, pk, pv, **kw)
    q, k, v, pk, pv = dense_operands(900, b, hq, hkv, 1, 1, t - 1, d)
    if name == "overflow_scores":  # query heads of KV head 0 and every third cached key of it in 2^[62,64]: |q.k| scale is beyond f32 there, finite elsewhere
        q[:, 0:g] = wide(rng, q[:, 0:g].shape, 62, 64)
        pk[:, 0, ::3] = wide(rng, pk[:, 0, ::3].shape, 62, 64)
    elif name == "one_survivor":  # depth 0 carries 20 * 60 / 8 = 150 into the survivor's score and nothing into any other
        q[..., 0] = 20.0
        pk[..., 0] = 0.0
        k[..., 0] = 0.0
        pk[:, :, SURVIVOR, 0] = 60.0
    elif name == "subnormal_p":  # V in 2^[-140,-120]: ordinary p ~ 2^-7 times v is subnormal; five keys at about max - 86: their p itself is subnormal
        pv = wide(rng, pv.shape, -140, -120)
        v = wide(rng, v.shape, -140, -120)
        q[..., 0] = 19.0
        pk[..., 0] = 0.0
        k[..., 0] = 0.0
        # the exponential is cut to 0 below ln(2^-126) = -87.3, so a subnormal p is exp(x - max) above that cut divided by the row's sum (about 100):
        # x - max in (-87.3, -82.7).  19 * c / 8 for c = -34 .. -36 is -80.8 .. -85.5, under a maximum of about 3
        pk[:, :, 10:15, 0] = np.linspace(-34.0, -36.0, 5, dtype=F)
    else:
        raise KeyError(name)
    return make(name, q, k, v, pk, pv, **kw)


def probabilities(c):
    """[B, Hq, T] probabilities of a one-row case as the rule computes them (before the NaN flush) and the raw scores."""
    assert c.sq == 1
    key = c.k if c.pk is None else np.concatenate([c.pk, c.k], axis=2)
    scale = float(F(1.0) / np.sqrt(F(c.d))) if c.scale is None else c.scale
    g = c.hq // c.hkv
    scores = np.empty((c.b, c.hq, c.t), F)
    with np.errstate(all="ignore"):
        for b in range(c.b):
            for h in range(c.hq):
                s = ref.gemm_f32(c.q[b, h], key[b, h // g].T, alpha=scale)[0]
                if c.mask is not None and c.mask.dtype == F:
                    s = s + np.broadcast_to(c.mask, (c.b, c.hq, 1, c.t))[b, h, 0]
                if c.nonpad is not None and not c.causal:
                    s[int(c.nonpad[b]):] = -np.inf
                scores[b, h] = s
        return ref.softmax(scores, flush_nan=False), scores


def shares(x):
    x = np.abs(np.asarray(x, np.float64)).reshape(-1)
    return dict(zero=float((x == 0).mean()), sub=float(((x > 0) & (x < TINY)).mean()), nan=float(np.isnan(x).mean()), inf=float(np.isinf(x).mean()),
                normal=float(((x >= TINY) & np.isfinite(x)).mean()))


def overflow_scores_holds(c, out):
    """Some scores of KV head 0's query heads are +-Inf and others finite (so the rows are NaN and flushed: those heads give zeros), the other heads ordinary."""
    _, scores = probabilities(c)
    g = c.hq // c.hkv
    hot, cold = shares(scores[:, :g]), shares(scores[:, g:])
    s = dict(hot=hot, cold=cold, flushed=shares(out[:, :g]), ordinary=shares(out[:, g:]))
    # (a third of the keys is drawn large: their scores are +-Inf, or NaN where a chain met Inf - Inf on the way)
    return hot["inf"] >= 0.05 and hot["inf"] + hot["nan"] >= 0.3 and hot["normal"] >= 0.6 and cold["normal"] == 1.0 and s["flushed"]["zero"] == 1.0 and \
        s["ordinary"]["normal"] >= 0.99, s


def one_survivor_holds(c, out):
    """The maximum exceeds every other score by more than 104: every other exponential is exactly 0, and the output is the survivor's V row."""
    p, scores = probabilities(c)
    rest = np.delete(scores, SURVIVOR, axis=2)
    s = dict(margin=float((scores[:, :, SURVIVOR:SURVIVOR + 1] - rest).min()), probs=shares(p))
    full = np.concatenate([c.pv, c.v], axis=2)
    same = np.array_equal(out[:, :, 0], np.repeat(full[:, :, SURVIVOR], c.hq // c.hkv, axis=1))
    return s["margin"] > 104 and s["probs"]["zero"] >= (c.t - 1) / c.t and same, s


def subnormal_p_holds(c, out):
    """At least one probability is subnormal, and at least a fifth of the terms p[t] * v[t, n] that the chains accumulate are subnormal and non-zero."""
    p, _ = probabilities(c)
    full = np.concatenate([c.pv, c.v], axis=2)
    with np.errstate(all="ignore"):
        terms = p[:, :, :, None] * np.repeat(full, c.hq // c.hkv, axis=1)
    s = dict(probs=shares(p), terms=shares(terms), out=shares(out))
    s["largest"] = float(np.abs(out).max())
    return s["probs"]["sub"] > 0 and s["terms"]["sub"] >= 0.2 and s["out"]["zero"] < 0.5 and s["out"]["nan"] == 0 and s["largest"] < 2.0 ** -110, s


def all_masked_holds(c, out):
    """Item 1's rows are all -inf (NaN after the softmax, flushed: exact zeros), item 0's are ordinary although its mask holds -inf entries."""
    p, scores = probabilities(c)
    s = dict(item1_scores=shares(scores[1]), item1_probs=shares(p[1]), item0=shares(out[0]), item1=shares(out[1]))
    return s["item1_scores"]["inf"] == 1.0 and s["item1_probs"]["nan"] == 1.0 and s["item1"]["zero"] == 1.0 and s["item0"]["normal"] >= 0.99 and \
        np.isinf(scores[0]).any(), s


HOLDS = {"overflow_scores": overflow_scores_holds, "one_survivor": one_survivor_holds, "subnormal_p": subnormal_p_holds, "all_masked": all_masked_holds}


def band_holds(name, out):
    """(holds, figures) for the rule's -- or any path's -- output (B, Hq, 1, Dv) of range_band(name)."""
    return HOLDS[name](range_band(name), np.asarray(out).reshape(range_band(name).o_shape))


def gqa_operands(c):
    """A one-row case as GroupQueryAttention's decode operands: q [B, 1, Hq * D], the LAST key / value row as k, v [B, 1, Hkv * D], the rows before it as the
    past, and what stands for the mask: an attention_bias [B, 1, 1, T] (item b all -inf where nonpad[b] is 0) -> (q, k, v, pk, pv, seqlens, total, bias)."""
    assert c.sq == 1 and c.d == c.dv and not c.causal
    key = c.k if c.pk is None else np.concatenate([c.pk, c.k], axis=2)
    val = c.v if c.pv is None else np.concatenate([c.pv, c.v], axis=2)
    flat = lambda x: np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(c.b, 1, -1)
    bias = None
    if c.mask is not None:
        bias = np.ascontiguousarray(np.broadcast_to(c.mask, (c.b, 1, 1, c.t))).copy()
        for b in range(c.b):
            assert c.nonpad is None or int(c.nonpad[b]) in (0, c.t)
            if c.nonpad is not None and int(c.nonpad[b]) == 0:
                bias[b] = -np.inf
    return flat(c.q), flat(key[:, :, -1:]), flat(val[:, :, -1:]), np.ascontiguousarray(key[:, :, :-1]), np.ascontiguousarray(val[:, :, :-1]), \
        [c.t - 1] * c.b, c.t, bias


# ------------------------------------------------------------------------------------------------ MatMulNBits: non-finite rows and columns
NBITS_NONFINITE_SHAPE = (65, 272, 130, 16)  # rows, K, N, block: a ragged tile in both directions, a 16-deep tail


def nbits_operands(lead, k, n, bs, seed=1234):
    """lhs [*lead, k] in [-0.5, 0.5), every code, scales in [0, 1) from the oracle's generator (tests/test_gpu_nbits_gemm.py::draw is this function)."""
    rng = ref.XorShiftRng(seed)
    lhs = (rng.f32(int(np.prod(lead)) * k) - F(0.5)).reshape(*lead, k)
    return lhs, rng.u8(n * (k // 2)).reshape(n, k // bs, bs // 2), rng.f32(n * (k // bs)).reshape(n, k // bs)


def nbits_nonfinite(lhs, scales):
    """lhs row 5 all NaN and +Inf in its last element; the scales of output column 7 all NaN and -Inf in the last scale -> (lhs, scales, dep [rows, N]): rows 5
    and rows - 1 and columns 7 and N - 1 depend on a non-finite value, nothing else does."""
    lhs, scales = lhs.copy(), scales.copy()
    m, n = lhs.shape[0], scales.shape[0]
    assert lhs.ndim == 2 and m > 6 and n > 8
    lhs[5] = np.nan
    lhs[m - 1, -1] = np.inf
    scales[7] = np.nan
    scales[n - 1, -1] = -np.inf
    dep = np.zeros((m, n), bool)
    dep[[5, m - 1]] = True
    dep[:, [7, n - 1]] = True
    return lhs, scales, dep
