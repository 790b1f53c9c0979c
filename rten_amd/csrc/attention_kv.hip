// Attention (ai.onnx, opset 23) with past_key / past_value inputs and present outputs: Attention::run_impl, src/ops/attention.rs:579-973, on sdpa_head
// (attention.rs:518-562) and concat_past_kv (attention.rs:470-507).
//
//   present = concat(past, current) on axis 2 (the current K / V when there is no past);  T = past_seq + kv_seq is a host-known shape
//   out[b, h] = softmax(mod(scale * Q[b, h] present_k[b, h / G]^T)) present_v[b, h / G],  G = Hq / Hkv; every product has T columns / T depth
//   mod, row q_idx, in this order (attention.rs:850-886):
//     1. a float mask is ADDED, an int32 (bool) mask OVERWRITES with -inf where it is 0; the mask is broadcast to (B, Hq, Sq, T) through four strides
//     2. is_causal: -inf from clamp(offset + q_idx + 1, 0, T) on, offset = nonpad[b] - Sq when nonpad_kv_seqlen is given, else past_seq
//     3. not causal, nonpad_kv_seqlen given: -inf on [nonpad[b], T)
//   then the three-pass softmax of rowwise.hip with NaN -> 0 (softmax_row.h).  Masked keys stay in both products with probability 0 (a NaN in a masked V
//   row propagates, as in the reference); a fully masked row gives zeros.
// The only device value is nonpad_kv_seqlen; it only masks, is clamped into [0, T] where it is read, and nothing is read back: a call captures and a
// replay follows new values.
//
// The kernels of this unit:
//   * attn_decode_kernel<D> (Sq == 1, gemv order on, D == Dv in {64, 128}, G <= 32): ONE launch, no prepare launch and no scratch.  One workgroup of 1024
//     threads per (batch, KV head) serves the G query heads of the group.  Key t is read from past_key when t < past_seq, else from row t - past_seq of
//     `key` through that input's strides (3-D and 4-D layouts alike), so the cache crosses HBM once in and, when present is wanted, once out:
//       - scores, the transposed-B one-row form of gemv_f32.hip: 16 lanes per key, lane l holds depths l + 16 j in D / 16 registers and stores them to
//         present_key from there; 16 lane accumulators folded +8, +4, +2, +1, then scale * acc; the < 8 keys left over in a column block of
//         max(128, ceil(T / gemv_threads)) keys take the scalar fmaf chain and acc * scale.  D <= 512: one depth block, no beta step.
//       - the score modification above, rows in LDS, then softmax_row, one wave per head.
//       - PV, the row-major-B one-row form: depth blocks of 8 keys, each an fmaf chain from zero; thread (column n, block slot sl) loads the 8 V elements
//         of its block ONCE, stores them to present_value, and chains them for every head of the group, 8 heads parked in LDS at a time; the thread that
//         owns (head, column) folds the parked sums in block order (first block stored, the rest added).  D is 64 or 128: no left-over columns.
//     LDS: 4 * (G * D [q] + 8192 [block sums: 1024 / D slots x 8 heads x D] + G * T [score rows]) bytes <= 160 KiB, the formula of gqa_decode_kernel.
//   * the split decode form (attention_split.hip; Sq == 1, gemv order on, D and Dv each 64 or 128, G <= 512, no LDS bound): the key range of one (batch, KV
//     head) spread over workgroups in four dependent launches, same arithmetic.  The rule takes it where the kernel above does not cover such a call, and where
//     B * Hkv workgroups under-fill the device at a cache long enough to pay for the extra launches (rten_attn_split_pays).
//   * the fused prefill kernel (attention_prefill.hip; more than one query row, or one row in the blocked order, D == Dv in {64, 128}): the composed path's
//     two products and its score kernel in one launch with no score buffer, same bits.  Mode 4, and mode 0 where prefill_pays() holds.
//   * attn_concat_kernel: present_key and present_value of the composed path in one launch (into scratch when the caller does not want them and the
//     GEMMs cannot read the inputs in place).
//   * attn_scores_kernel: the score modification and softmax_row on a scratch row, one wave per row, between the two GEMMs of the composed path (any D,
//     Dv, Sq): the group is the GEMMs' inner batch level with stride 0 on K and V; one query row takes the gemv entry on T columns (T is a shape here, so
//     which keys are a column block's left-overs is host-known), more rows rten_gemm_f32_blocked; the query rows are worked in passes of <= 64 MiB of scores.
#include "attention_common.h"
#include "softmax_row.h"

namespace {

constexpr int DEC_THREADS = 1024;
constexpr int DEC_HC = 8;    // heads whose block sums are parked at a time
constexpr int DEC_MAXCH = 4; // chunks of DEC_HC heads whose output an owner thread carries: G <= 32

template <int D>
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_kernel(const AttnArgs p) {
    extern __shared__ float smem[];
    constexpr int NS = DEC_THREADS / D; // depth blocks chained per round
    const int G = p.G, T = p.T, P = p.P;
    float *qs = smem;                      // [G][D]
    float *bs = qs + G * D;                // [NS][DEC_HC][D]
    float *sc = bs + DEC_THREADS * DEC_HC; // [G][T]
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int from = masked_from(p, nonpad_of(p, b), 0);
    const float *q = p.q + b * p.q_sb + (int64_t)g * G * p.q_sh;
    for (int i = tid; i < G * D; i += DEC_THREADS) qs[i] = q[(i / D) * p.q_sh + (i % D)];
    __syncthreads();

    // ---- scores: 16 lanes per key, 64 keys per pass; the key row goes from the registers to present_key
    long long cbl = 128;
    if (p.gemv_threads > 0) {
        cbl = ((long long)T + p.gemv_threads - 1) / p.gemv_threads;
        if (cbl < 128) cbl = 128;
    }
    const int cb = (int)(cbl > 0x7fffffff ? 0x7fffffff : cbl);
    const float *past_k = p.past_k + ((int64_t)b * p.Hkv + g) * P * D; // (never dereferenced when P == 0)
    const float *new_k = p.k + b * p.k_sb + g * p.k_sh;
    float *pk = p.pk ? p.pk + ((int64_t)b * p.Hkv + g) * T * D : nullptr;
    const int l = tid & 15, grp = tid >> 4;
    for (int t0 = 0; t0 < T; t0 += DEC_THREADS / 16) {
        const int t = t0 + grp;
        const bool live = t < T;
        const int tt = live ? t : T - 1;
        const int c0 = tt / cb * cb, nc = T - c0 < cb ? T - c0 : cb;
        const bool vec = (tt - c0) < nc / 8 * 8; // else: a left-over key of its column block -> the scalar chain
        const float *kr = tt < P ? past_k + (int64_t)tt * D : new_k + (tt - P) * p.k_ss;
        float kreg[D / 16];
#pragma unroll
        for (int j = 0; j < D / 16; j++) kreg[j] = kr[l + 16 * j];
        if (pk && live) {
#pragma unroll
            for (int j = 0; j < D / 16; j++) pk[(int64_t)t * D + l + 16 * j] = kreg[j];
        }
        for (int h = 0; h < G; h++) {
            const float *qh = qs + h * D;
            float part = 0.f;
#pragma unroll
            for (int j = 0; j < D / 16; j++) part = fmaf(qh[l + 16 * j], kreg[j], part);
            part = part + __shfl_down(part, 8, 16);
            part = part + __shfl_down(part, 4, 16);
            part = part + __shfl_down(part, 2, 16);
            part = part + __shfl_down(part, 1, 16);
            if (live && l == 0) {
                float o = p.scale * part;
                if (!vec) {
                    float acc = 0.f;
                    for (int k = 0; k < D; k++) acc = fmaf(qh[k], kr[k], acc);
                    o = acc * p.scale;
                }
                sc[h * T + t] = modified(p, o, mask_row(p, b, g * G + h, 0), t, from);
            }
        }
    }
    __syncthreads();

    // ---- softmax: one wave per head
    for (int h = tid >> 6; h < G; h += DEC_THREADS / 64) softmax_row(sc + h * T, T, tid & 63);
    __syncthreads();

    // ---- PV: thread = (column n, block slot sl) loads its block of V once (and stores it to present_value), then chains it for 8 heads at a time; the
    // owner of (head hh, column nn) of each chunk folds the parked block sums in block order
    const int n = tid % D, sl = tid / D;
    const int hh_own = tid / D, nn_own = tid % D; // (DEC_HC * D <= DEC_THREADS)
    const float *past_v = p.past_v + ((int64_t)b * p.Hkv + g) * P * D;
    const float *new_v = p.v + b * p.v_sb + g * p.v_sh;
    float *pv = p.pv ? p.pv + ((int64_t)b * p.Hkv + g) * T * D : nullptr;
    const int nblk = (T + 7) / 8;
    const int nch = (G + DEC_HC - 1) / DEC_HC;
    float o[DEC_MAXCH];
#pragma unroll
    for (int c = 0; c < DEC_MAXCH; c++) o[c] = 0.f;
    for (int blk0 = 0; blk0 < nblk; blk0 += NS) {
        const int blk = blk0 + sl;
        const int k0 = blk * 8;
        const int depth = blk < nblk ? (T - k0 < 8 ? T - k0 : 8) : 0;
        float vv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            vv[k] = 0.f;
            if (k < depth) {
                const int t = k0 + k;
                vv[k] = t < P ? past_v[(int64_t)t * D + n] : new_v[(t - P) * p.v_ss + n];
                if (pv) pv[(int64_t)t * D + n] = vv[k];
            }
        }
        const int cnt = nblk - blk0 < NS ? nblk - blk0 : NS;
#pragma unroll
        for (int c = 0; c < DEC_MAXCH; c++) {
            if (c < nch) { // (uniform over the workgroup: the barriers below are reached by every thread)
                const int hc0 = c * DEC_HC;
                const int nh = G - hc0 < DEC_HC ? G - hc0 : DEC_HC;
#pragma unroll
                for (int hh = 0; hh < DEC_HC; hh++) {
                    float acc = 0.f;
                    if (hh < nh) {
                        const float *pr = sc + (hc0 + hh) * T + k0;
#pragma unroll
                        for (int k = 0; k < 8; k++)
                            if (k < depth) acc = fmaf(pr[k], vv[k], acc);
                    }
                    bs[(sl * DEC_HC + hh) * D + n] = acc;
                }
                __syncthreads();
                if (hh_own < nh) {
                    for (int s2 = 0; s2 < cnt; s2++) {
                        const float v = bs[(s2 * DEC_HC + hh_own) * D + nn_own];
                        o[c] = (blk0 + s2 == 0) ? v : o[c] + v; // the first block is stored, the rest are added
                    }
                }
                __syncthreads();
            }
        }
    }
    float *outb = p.out + b * p.o_sb + (int64_t)g * G * p.o_sh;
#pragma unroll
    for (int c = 0; c < DEC_MAXCH; c++)
        if (c < nch && c * DEC_HC + hh_own < G && hh_own < DEC_HC) outb[(c * DEC_HC + hh_own) * p.o_sh + nn_own] = o[c];
}

// composed path: present[b, g, t, :] = t < P ? past[b, g, t, :] : current[b, g, t - P, :] for K (D wide) and V (Dv wide) in one launch
__global__ __launch_bounds__(256) void attn_concat_kernel(const AttnArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nk = (int64_t)p.B * p.Hkv * p.T * p.D, nv = (int64_t)p.B * p.Hkv * p.T * p.Dv;
    if (idx >= nk + nv) return;
    const bool is_v = idx >= nk;
    const int w = is_v ? p.Dv : p.D;
    int64_t e = is_v ? idx - nk : idx;
    const int d = (int)(e % w);
    e /= w;
    const int t = (int)(e % p.T);
    e /= p.T;
    const int g = (int)(e % p.Hkv), b = (int)(e / p.Hkv);
    float val;
    if (t < p.P) val = (is_v ? p.past_v : p.past_k)[(((int64_t)b * p.Hkv + g) * p.P + t) * w + d];
    else if (is_v) val = p.v[b * p.v_sb + g * p.v_sh + (t - p.P) * p.v_ss + d];
    else val = p.k[b * p.k_sb + g * p.k_sh + (t - p.P) * p.k_ss + d];
    (is_v ? p.pv : p.pk)[is_v ? idx - nk : idx] = val;
}

// composed path: score modification + softmax on row (b, h, s0 + i) of this pass's scores [B, Hq, SC, T], one wave per row
__global__ __launch_bounds__(256) void attn_scores_kernel(const AttnArgs p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)p.B * p.Hq * p.SC) return;
    const int s = p.s0 + (int)(row % p.SC);
    const int64_t bh = row / p.SC;
    const int h = (int)(bh % p.Hq), b = (int)(bh / p.Hq);
    const int from = masked_from(p, nonpad_of(p, b), s);
    const void *mrow = mask_row(p, b, h, s);
    float *r = p.scores + row * p.T;
    for (int i = lane; i < p.T; i += 64) r[i] = modified(p, r[i], mrow, i, from);
    softmax_row(r, p.T, lane);
}

size_t decode_lds_bytes(int G, int D, int T) { return sizeof(float) * ((size_t)G * D + (size_t)DEC_THREADS * DEC_HC + (size_t)G * T); }
constexpr size_t LDS_PER_WORKGROUP = 160 * 1024;
constexpr size_t SCORE_PASS_BYTES = 64u << 20; // the composed path's score buffer per pass over the query rows

// Whether mode 0 prefers the fused prefill kernel (attention_prefill.hip) to the composed path for a call that kernel covers: the measured range of
// docs/KERNELS.md 4.19.  Causal first prompts (no past, as many rows as keys) without a mask, from 8192 keys at head size 128 (20.1 against 35.0 ms at
// Hq 32 / Hkv 8) and from 2048 keys at head size 64 (0.96 against 1.07 ms), on at least the 1024 workgroups of the smaller of those two rows.  It loses
// at 128 .. 2048 keys at head size 128, on the chunked prompt and on the non-causal one: those stay on the composed path.
bool prefill_pays(const AttnArgs &a) {
    if (!a.causal || a.P != 0 || a.Sq != a.T || a.mask_kind != RTEN_HIP_ATTN_MASK_NONE) return false;
    if ((int64_t)a.B * a.Hq * ((a.Sq + 63) / 64) < 1024) return false;
    return a.D == 128 ? a.T >= 8192 : a.T >= 2048;
}

template <int D>
int32_t launch_decode(rten_hip_ctx *ctx, const AttnArgs &a, size_t lds) {
    // the kernel's dynamic LDS ceiling, raised once per device (not a stream operation: nothing lands in a capture)
    static std::once_flag raised[64];
    static hipError_t raised_rc[64];
    const int dev = ctx->device & 63;
    std::call_once(raised[dev], [&] {
        raised_rc[dev] = hipFuncSetAttribute((const void *)attn_decode_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_PER_WORKGROUP);
    });
    RTEN_HIP_TRY(ctx, raised_rc[dev]);
    const double kvb = 8.0 * a.B * a.Hkv * (double)a.T * D;
    ProfScope ps(ctx, "attn_decode_kernel", 4.0 * a.B * a.Hq * (double)a.T * D, (a.pk ? 2.0 : 1.0) * kvb + 8.0 * a.B * a.Hq * D);
    hipLaunchKernelGGL(attn_decode_kernel<D>, dim3((unsigned)a.Hkv, (unsigned)a.B), dim3(DEC_THREADS), lds, ctx->stream, a);
    RTEN_LAUNCH_CHECK(ctx, "attn_decode_kernel");
    return RTEN_HIP_OK;
}

} // namespace

RTEN_EXPORT int32_t rten_hip_set_attention_path(rten_hip_ctx *ctx, int32_t mode) {
    RTEN_CHECK_CTX(ctx);
    if (mode < 0 || mode > 4) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "set_attention_path: mode must be 0 .. 4");
    ctx->attention_path = mode;
    return RTEN_HIP_OK;
}

RTEN_EXPORT int32_t rten_hip_set_attention_split(rten_hip_ctx *ctx, int32_t keys_per_workgroup) {
    RTEN_CHECK_CTX(ctx);
    if (keys_per_workgroup < 0 || keys_per_workgroup % 8 != 0)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "set_attention_split: keys_per_workgroup must be 0 (the rule) or a positive multiple of 8");
    ctx->attention_split = keys_per_workgroup;
    return RTEN_HIP_OK;
}

RTEN_EXPORT int32_t rten_hip_attention_f32(rten_hip_ctx *ctx, const int32_t *dims, const int64_t *strides, float scale, const float *q, const float *k,
                                           const float *v, const void *attn_mask, const float *past_key, const float *past_value,
                                           const int32_t *nonpad_kv_seqlen, float *out, float *present_key, float *present_value) {
    RTEN_CHECK_CTX(ctx);
    if (!dims || !strides) return RTEN_HIP_ERR_INVALID_VALUE;
    AttnArgs a = {};
    a.B = dims[0]; a.Hq = dims[1]; a.Hkv = dims[2]; a.Sq = dims[3]; a.Skv = dims[4]; a.P = dims[5]; a.D = dims[6]; a.Dv = dims[7];
    a.causal = dims[8] != 0; a.mask_kind = dims[9];
    if (a.B < 0 || a.Hq <= 0 || a.Hkv <= 0 || a.Sq < 0 || a.Skv < 0 || a.P < 0 || a.D < 0 || a.Dv < 0 || a.Hq % a.Hkv != 0) return RTEN_HIP_ERR_INVALID_VALUE;
    if (a.mask_kind < RTEN_HIP_ATTN_MASK_NONE || a.mask_kind > RTEN_HIP_ATTN_MASK_BOOL) return RTEN_HIP_ERR_INVALID_VALUE;
    if ((int64_t)a.P + a.Skv > 0x7fffffff) return RTEN_HIP_ERR_INVALID_VALUE;
    a.T = a.P + a.Skv; a.G = a.Hq / a.Hkv;
    if (a.B == 0) return RTEN_HIP_OK;
    if (a.T == 0 || a.D == 0 || a.Dv == 0 || a.Sq == 0)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "attention: an empty query, key range or head is not supported");
    if (!q || !k || !v || !out) return RTEN_HIP_ERR_INVALID_VALUE;
    if (a.P > 0 && (!past_key || !past_value)) return RTEN_HIP_ERR_INVALID_VALUE;
    if ((a.mask_kind != RTEN_HIP_ATTN_MASK_NONE) != (attn_mask != nullptr)) return RTEN_HIP_ERR_INVALID_VALUE;
    if ((present_key == nullptr) != (present_value == nullptr)) return RTEN_HIP_ERR_INVALID_VALUE;
    a.q_sb = strides[0]; a.q_sh = strides[1]; a.q_ss = strides[2];
    a.k_sb = strides[3]; a.k_sh = strides[4]; a.k_ss = strides[5];
    a.v_sb = strides[6]; a.v_sh = strides[7]; a.v_ss = strides[8];
    a.o_sb = strides[9]; a.o_sh = strides[10]; a.o_ss = strides[11];
    a.m_sb = strides[12]; a.m_sh = strides[13]; a.m_sq = strides[14]; a.m_st = strides[15];
    for (int i = 0; i < RTEN_HIP_ATTENTION_NSTRIDES; i++)
        if (strides[i] < 0) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "attention: negative strides are not supported");
    a.q = q; a.k = k; a.v = v; a.past_k = past_key; a.past_v = past_value; a.mask = attn_mask; a.nonpad = nonpad_kv_seqlen;
    a.pk = present_key; a.pv = present_value; a.out = out; a.scale = scale;
    a.gemv_threads = ctx->gemv_threads;

    const bool one_row = a.Sq == 1 && ctx->gemv_order != 0;
    const char *const prefill_cover = "attention: the fused prefill kernel takes more than one query row, or one row with the gemv order off, equal K and V head sizes of 64 or 128, and 16-byte aligned K and V";
    if (ctx->attention_path == 4 && (one_row || !rten_attn_prefill_covers(a))) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, prefill_cover);
    const size_t lds = decode_lds_bytes(a.G, a.D, a.T);
    const bool covered = one_row && a.D == a.Dv && (a.D == 64 || a.D == 128) && a.G <= DEC_HC * DEC_MAXCH && lds <= LDS_PER_WORKGROUP;
    if (ctx->attention_path == 2 && !covered)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "attention: the decode kernel takes one query row in the gemv order, equal K and V head sizes of 64 or 128, at most 32 query heads per KV head and rows that fit LDS");
    const bool splittable = one_row && rten_attn_split_covers(a);
    if (ctx->attention_path == 3 && !splittable)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "attention: the split decode form takes one query row in the gemv order, K and V head sizes of 64 or 128 and at most 512 query heads per KV head");
    if (splittable && (ctx->attention_path == 3 || (ctx->attention_path == 0 && (!covered || rten_attn_split_pays(ctx, a)))))
        return rten_attn_split_launch(ctx, a, ctx->attention_split);
    if (covered && ctx->attention_path != 1) return a.D == 64 ? launch_decode<64>(ctx, a, lds) : launch_decode<128>(ctx, a, lds);

    // ---- the fused prefill kernel and the composed path.  K and V are read in place when there is no past and the inputs are contiguous (B, Hkv, T, *);
    // otherwise out of present, or out of scratch when the caller does not want present.  Scratch (the auxiliary buffer: the GEMMs called below own
    // `scratch`): [K | V | scores]; the prefill kernel has no scores and needs none when K and V are read in place or present is supplied.
    const bool in_place = a.P == 0 && a.k_ss == a.D && a.k_sh == (int64_t)a.T * a.D && a.k_sb == (int64_t)a.Hkv * a.T * a.D && a.v_ss == a.Dv &&
                          a.v_sh == (int64_t)a.T * a.Dv && a.v_sb == (int64_t)a.Hkv * a.T * a.Dv;
    const size_t nk = (size_t)a.B * a.Hkv * a.T * a.D, nv = (size_t)a.B * a.Hkv * a.T * a.Dv;
    const bool own_kv = !in_place && !a.pk;
    const size_t kv_pad = own_kv ? (nk + 63) / 64 * 64 + (nv + 63) / 64 * 64 : 0;
    auto al16 = [](const void *ptr) { return ((uintptr_t)ptr & 15u) == 0; };
    const bool kv_al16 = in_place ? al16(a.k) && al16(a.v) : (own_kv || (al16(a.pk) && al16(a.pv)));
    const bool fusable = !one_row && rten_attn_prefill_covers(a) && kv_al16;
    if (ctx->attention_path == 4 && !fusable) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, prefill_cover);
    if (fusable && (ctx->attention_path == 4 || (ctx->attention_path == 0 && prefill_pays(a)))) {
        if (own_kv) {
            float *aux = (float *)rten_aux_scratch(ctx, kv_pad * sizeof(float) + 256);
            if (!aux) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "attention: scratch allocation failed (warm up before capture)");
            a.pk = aux + 64;
            a.pv = a.pk + (nk + 63) / 64 * 64;
        }
        if (a.pk) {
            ProfScope ps(ctx, "attn_concat_kernel", 0.0, 8.0 * (double)(nk + nv));
            hipLaunchKernelGGL(attn_concat_kernel, dim3((unsigned)ceil_div64((int64_t)(nk + nv), 256)), dim3(256), 0, ctx->stream, a);
            RTEN_LAUNCH_CHECK(ctx, "attn_concat_kernel");
        }
        return rten_attn_prefill_launch(ctx, a, in_place ? a.k : a.pk, in_place ? a.v : a.pv);
    }
    const size_t row_elems = (size_t)a.B * a.Hq * (size_t)a.T; // one query row of every (batch, head)
    size_t sc_rows = SCORE_PASS_BYTES / sizeof(float) / row_elems;
    sc_rows = sc_rows < 1 ? 1 : (sc_rows > (size_t)a.Sq ? (size_t)a.Sq : sc_rows);
    a.SC = (int)sc_rows;
    float *aux = (float *)rten_aux_scratch(ctx, (kv_pad + row_elems * sc_rows) * sizeof(float) + 256);
    if (!aux) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "attention: scratch allocation failed (warm up before capture)");
    aux += 64;
    if (own_kv) { a.pk = aux; a.pv = aux + (nk + 63) / 64 * 64; }
    a.scores = aux + kv_pad;
    if (a.pk) {
        ProfScope ps(ctx, "attn_concat_kernel", 0.0, 8.0 * (double)(nk + nv));
        hipLaunchKernelGGL(attn_concat_kernel, dim3((unsigned)ceil_div64((int64_t)(nk + nv), 256)), dim3(256), 0, ctx->stream, a);
        RTEN_LAUNCH_CHECK(ctx, "attn_concat_kernel");
    }
    const float *kc = in_place ? a.k : a.pk, *vc = in_place ? a.v : a.pv;

    // Batch levels: outer = (b, KV head), inner = the G query heads of the group, K and V with inner stride 0.  (b, KV head) is one stride of Q and out
    // only for one batch item, or when their batch stride is Hq heads (the 4-D layout; one token of the 3-D layout); otherwise one launch per batch item.
    const bool merged = a.B == 1 || (a.q_sb == (int64_t)a.Hq * a.q_sh && a.o_sb == (int64_t)a.Hq * a.o_sh);
    const int launches = merged ? 1 : a.B;
    const int outer = merged ? a.B * a.Hkv : a.Hkv;
    auto gemm = [&](const rten_hip_gemm_desc &g, const float *x, const float *y, float *z) {
        return one_row ? rten_hip_gemm_f32(ctx, &g, x, y, nullptr, z) : rten_gemm_f32_blocked(ctx, &g, x, y, nullptr, z);
    };
    for (a.s0 = 0; a.s0 < a.Sq; a.s0 += a.SC) {
        if (a.Sq - a.s0 < a.SC) a.SC = a.Sq - a.s0;
        const int64_t score_b = (int64_t)a.Hq * a.SC * a.T;
        for (int i = 0; i < launches; i++) { // scores = scale * Q K^T
            rten_hip_gemm_desc g = {};
            g.m = a.SC; g.n = a.T; g.k = a.D;
            g.a_rs = a.q_ss; g.a_cs = 1; g.b_rs = 1; g.b_cs = a.D; g.ldc = a.T;
            g.batch = outer * a.G; g.batch_inner = a.G;
            g.a_bs = (int64_t)a.G * a.q_sh; g.a_bsi = a.q_sh;
            g.b_bs = (int64_t)a.T * a.D; g.b_bsi = 0;
            g.c_bs = (int64_t)a.G * a.SC * a.T; g.c_bsi = (int64_t)a.SC * a.T;
            g.alpha = a.scale; g.beta = 0.f;
            const int32_t rc = gemm(g, a.q + i * a.q_sb + a.s0 * a.q_ss, kc + (int64_t)i * a.Hkv * a.T * a.D, a.scores + i * score_b);
            if (rc) return rc;
        }
        {
            const int64_t rows = (int64_t)a.B * a.Hq * a.SC;
            ProfScope ps(ctx, "attn_scores_kernel", 0.0, 8.0 * rows * a.T);
            hipLaunchKernelGGL(attn_scores_kernel, dim3((unsigned)ceil_div64(rows, 4)), dim3(256), 0, ctx->stream, a);
            RTEN_LAUNCH_CHECK(ctx, "attn_scores_kernel");
        }
        for (int i = 0; i < launches; i++) { // out = P V
            rten_hip_gemm_desc g = {};
            g.m = a.SC; g.n = a.Dv; g.k = a.T;
            g.a_rs = a.T; g.a_cs = 1; g.b_rs = a.Dv; g.b_cs = 1; g.ldc = a.o_ss;
            g.batch = outer * a.G; g.batch_inner = a.G;
            g.a_bs = (int64_t)a.G * a.SC * a.T; g.a_bsi = (int64_t)a.SC * a.T;
            g.b_bs = (int64_t)a.T * a.Dv; g.b_bsi = 0;
            g.c_bs = (int64_t)a.G * a.o_sh; g.c_bsi = a.o_sh;
            g.alpha = 1.f; g.beta = 0.f;
            const int32_t rc = gemm(g, a.scores + i * score_b, vc + (int64_t)i * a.Hkv * a.T * a.Dv, a.out + i * a.o_sb + a.s0 * a.o_ss);
            if (rc) return rc;
        }
    }
    return RTEN_HIP_OK;
}
