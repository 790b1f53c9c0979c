// Attention (ai.onnx, opset 23) decode (Sq == 1, gemv order on, D and Dv each 64 or 128, G <= 512) with the key range of one (batch, KV head) spread over
// many workgroups.  The arithmetic is that of attn_decode_kernel (attention_kv.hip), order for order, so every split gives the bits of
// tests/attention_rules.py; what changes is where a value lives: score rows and 8-key block sums sit in device scratch instead of LDS, so no row has to fit
// a workgroup, a batch-1 call fills the device, and the present stores are spread over every compute unit instead of B * Hkv of them.
//
// Four dependent launches on the stream, none of which only prepares: the cache is appended inside the two launches that read it.  No workgroup waits on
// another, there is no counter and nothing to restore, so a captured call replays.  A "unit" is one (batch, KV head); a "chunk" is keys_per_workgroup keys (a
// multiple of 8, so no 8-key depth block straddles two workgroups).  T = past_seq + kv_seq is a shape: the number of chunks, the column block and so which
// keys are its left-overs are host arithmetic, and no workgroup is launched to exit.  The only device value, nonpad_kv_seqlen, masks and nothing else.
//   1. attn_split_scores_kernel<D>, 256 threads per (unit, chunk): key t comes from past_key when t < P, else from row t - P of `key` through that input's
//      strides (a chunk may straddle the boundary).  16 lanes per key, lane l holds depths l + 16 j in D / 16 registers, stores them to present_key (first
//      walk only) and dots them with the query rows parked in LDS, 16 heads at a time (8 KiB whatever G is; a group of more than 16 heads walks its K chunk
//      again out of cache); the fold is + 8, + 4, + 2, + 1, then scale * acc; the < 8 left-over keys of a column block take the scalar fmaf chain and
//      acc * scale.  Then the score modification, into the scratch row.
//   2. attn_split_softmax_kernel, 1024 threads per score row: split_softmax_row (split_rows.h, shared with gqa_split.hip) with the row length T.
//   3. attn_split_pv_kernel<Dv>, 256 threads per (unit, chunk): thread = (output column, block slot).  p = e * (1 / sum), NaN -> 0, is rounded once per
//      (head, key) into an LDS tile of 16 KiB (4096 / G keys at a time).  For each 8-key depth block the thread loads its 8 V elements once (past_value or
//      `value`, by the rule of K), stores them to present_value, and chains them from zero for every head of the group with the probabilities read from LDS as
//      a broadcast.  Block sums go to scratch [row, ceil(T / 8), Dv].  Full blocks take a branch-free path.  Masked keys stay in the chains with probability
//      0: a NaN in such a V row propagates, as in the rule.
//   4. attn_split_fold_kernel, 256 threads per (row, 32 output columns): split_fold_row (split_rows.h), into `out` through its strides.
// D and Dv belong to different kernels, so they are independent.
//
// Scratch (floats, rten_aux_scratch), a function of host-known dims only.  With Tp = T rounded up to 64 and NB = ceil(T / 8), one unit needs
// G * (Tp + NB * Dv) floats.  The units are worked through in passes of U = clamp(64 MiB / unit bytes, 1, B * Hkv) units, and the buffer is
// round_up(U * G, 64) [1 / sum]  +  U * G * Tp [score rows]  +  U * G * NB * Dv [block sums].
#include "attention_common.h"
#include "split_rows.h"

namespace {

constexpr int SPL_THREADS = 256;
constexpr int SPL_QH = 16;    // query heads parked in LDS at a time
constexpr int PV_TILE = 4096; // probabilities parked in LDS at a time (floats): 8-key blocks of the G heads
constexpr size_t SPLIT_PASS_BYTES = 64u << 20;

struct SplitArgs {
    AttnArgs p;
    float *inv, *e, *bs; // [U * G], [U * G, Tp], [U * G, NB, Dv]
    int u0;              // first unit of this pass
    int ck, nchunks, Tp, NB;
    int cb;              // the gemv order's column block: max(128, ceil(T / gemv_threads)) keys
};

template <int D>
__global__ __launch_bounds__(SPL_THREADS) void attn_split_scores_kernel(const SplitArgs s) {
    __shared__ float qs[SPL_QH * D];
    const AttnArgs &p = s.p;
    const int tid = threadIdx.x, G = p.G, T = p.T, P = p.P, cb = s.cb;
    const int ul = blockIdx.x / s.nchunks, b = (s.u0 + ul) / p.Hkv, g = (s.u0 + ul) % p.Hkv;
    const int t_lo = (blockIdx.x % s.nchunks) * s.ck, t_hi = T - t_lo < s.ck ? T : t_lo + s.ck; // (nchunks = ceil(T / ck): t_lo < T)
    const int from = masked_from(p, nonpad_of(p, b), 0);
    const float *past_k = p.past_k + ((int64_t)b * p.Hkv + g) * P * D; // (never dereferenced when P == 0)
    const float *new_k = p.k + b * p.k_sb + g * p.k_sh;
    float *pk = p.pk ? p.pk + ((int64_t)b * p.Hkv + g) * T * D : nullptr;
    const int l = tid & 15, grp = tid >> 4;
    for (int h0 = 0; h0 < G; h0 += SPL_QH) {
        const int nh = G - h0 < SPL_QH ? G - h0 : SPL_QH;
        const float *q = p.q + b * p.q_sb + ((int64_t)g * G + h0) * p.q_sh;
        if (h0) __syncthreads();
        for (int i = tid; i < nh * D; i += SPL_THREADS) qs[i] = q[(i / D) * p.q_sh + (i % D)];
        __syncthreads();
        float *xr = s.e + ((int64_t)ul * G + h0) * s.Tp;
        for (int t0 = t_lo; t0 < t_hi; t0 += SPL_THREADS / 16) {
            const int t = t0 + grp;
            const bool live = t < t_hi;
            const int tt = live ? t : t_hi - 1;
            const int c0 = tt / cb * cb, nc = T - c0 < cb ? T - c0 : cb;
            const bool vec = (tt - c0) < nc / 8 * 8; // else: a left-over key of its column block -> the scalar chain
            const float *kr = tt < P ? past_k + (int64_t)tt * D : new_k + (tt - P) * p.k_ss;
            float kreg[D / 16];
#pragma unroll
            for (int j = 0; j < D / 16; j++) kreg[j] = kr[l + 16 * j];
            if (pk && live && h0 == 0) {
#pragma unroll
                for (int j = 0; j < D / 16; j++) pk[(int64_t)t * D + l + 16 * j] = kreg[j];
            }
            for (int h = 0; h < nh; h++) {
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
                    xr[(int64_t)h * s.Tp + t] = modified(p, o, mask_row(p, b, g * G + h0 + h, 0), t, from);
                }
            }
        }
    }
}

__global__ __launch_bounds__(SM_THREADS) void attn_split_softmax_kernel(const SplitArgs s) {
    const int row = blockIdx.x;
    split_softmax_row(s.e + (int64_t)row * s.Tp, s.p.T, s.inv + row);
}

// One 8-key depth block at key k0 of column n for the G heads: the V elements are loaded once (key t from the past when t < P, else from the new rows),
// stored to present_value when wanted, then chained from zero per head with the probabilities from LDS (row stride kt).
template <bool FULL>
__device__ __forceinline__ void block_sums(const float *past_v, const float *new_v, int64_t v_ss, int Dv, int P, float *pv, int k0, int depth, const float *pr,
                                           int kt, int G, float *dst, int64_t dst_stride) {
    float vv[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int t = k0 + k;
        vv[k] = (FULL || k < depth) ? (t < P ? past_v[(int64_t)t * Dv] : new_v[(t - P) * v_ss]) : 0.f;
    }
    if (pv) {
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (FULL || k < depth) pv[(int64_t)(k0 + k) * Dv] = vv[k];
    }
    for (int h = 0; h < G; h++) {
        const float4 p0 = *reinterpret_cast<const float4 *>(pr + h * kt), p1 = *reinterpret_cast<const float4 *>(pr + h * kt + 4);
        const float pp[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (FULL || k < depth) acc = fmaf(pp[k], vv[k], acc);
        dst[h * dst_stride] = acc;
    }
}

template <int DV>
__global__ __launch_bounds__(SPL_THREADS) void attn_split_pv_kernel(const SplitArgs s) {
    constexpr int NS = SPL_THREADS / DV; // depth blocks chained side by side
    __shared__ __attribute__((aligned(16))) float ps[PV_TILE];
    const AttnArgs &p = s.p;
    const int tid = threadIdx.x, G = p.G, T = p.T, P = p.P;
    const int ul = blockIdx.x / s.nchunks, b = (s.u0 + ul) / p.Hkv, g = (s.u0 + ul) % p.Hkv;
    const int t_lo = (blockIdx.x % s.nchunks) * s.ck, t_hi = T - t_lo < s.ck ? T : t_lo + s.ck;
    const int n = tid % DV, sl = tid / DV;
    const float *past_v = p.past_v + ((int64_t)b * p.Hkv + g) * P * DV + n; // (never dereferenced when P == 0)
    const float *new_v = p.v + b * p.v_sb + g * p.v_sh + n;
    float *pv = p.pv ? p.pv + ((int64_t)b * p.Hkv + g) * T * DV + n : nullptr;
    const int64_t row0 = (int64_t)ul * G;
    const int kt = PV_TILE / G / 8 * 8; // keys whose probabilities are parked at a time (the host refuses G > PV_TILE / 8)
    for (int k_lo = t_lo; k_lo < t_hi; k_lo += kt) {
        const int k_hi = t_hi - k_lo < kt ? t_hi : k_lo + kt;
        if (k_lo != t_lo) __syncthreads();
        for (int h = 0; h < G; h++) { // p = e * (1 / sum), NaN -> 0: rounded once per (head, key), before it enters a chain
            const float *er = s.e + (row0 + h) * s.Tp + k_lo;
            const float inv = s.inv[row0 + h];
            for (int k = tid; k < k_hi - k_lo; k += SPL_THREADS) {
                float r = er[k] * inv;
                if (!(r == r)) r = 0.f; // flush_nans_to_zero (attention.rs:551)
                ps[h * kt + k] = r;
            }
        }
        __syncthreads();
        for (int blk = k_lo / 8 + sl; blk * 8 < k_hi; blk += NS) {
            const int k0 = blk * 8, depth = T - k0;
            float *dst = s.bs + (row0 * s.NB + blk) * DV + n;
            if (depth >= 8) block_sums<true>(past_v, new_v, p.v_ss, DV, P, pv, k0, 8, ps + (k0 - k_lo), kt, G, dst, (int64_t)s.NB * DV);
            else block_sums<false>(past_v, new_v, p.v_ss, DV, P, pv, k0, depth, ps + (k0 - k_lo), kt, G, dst, (int64_t)s.NB * DV);
        }
    }
}

__global__ __launch_bounds__(256) void attn_split_fold_kernel(const SplitArgs s) {
    const AttnArgs &p = s.p;
    const int Dv = p.Dv, slices = Dv / FOLD_COLS;
    const int row = blockIdx.x / slices, cs = blockIdx.x % slices * FOLD_COLS;
    const int u = s.u0 + row / p.G, b = u / p.Hkv, g = u % p.Hkv;
    split_fold_row(s.bs + (int64_t)row * s.NB * Dv + cs, s.NB, Dv, p.out + b * p.o_sb + ((int64_t)g * p.G + row % p.G) * p.o_sh + cs);
}

struct SplitPlan {
    int Tp, NB, units, per_pass;
    size_t inv_elems, e_elems, bs_elems;
};

SplitPlan plan_of(const AttnArgs &a) {
    SplitPlan pl;
    pl.Tp = (int)(((int64_t)a.T + 63) / 64 * 64);
    pl.NB = (int)(((int64_t)a.T + 7) / 8);
    pl.units = a.B * a.Hkv;
    const size_t unit_bytes = sizeof(float) * (size_t)a.G * ((size_t)pl.Tp + (size_t)pl.NB * a.Dv);
    size_t per = SPLIT_PASS_BYTES / unit_bytes;
    per = per < 1 ? 1 : (per > (size_t)pl.units ? (size_t)pl.units : per);
    pl.per_pass = (int)per;
    pl.inv_elems = (per * a.G + 63) / 64 * 64;
    pl.e_elems = per * a.G * pl.Tp;
    pl.bs_elems = per * a.G * (size_t)pl.NB * a.Dv;
    return pl;
}

int32_t launch_pass(rten_hip_ctx *ctx, const SplitArgs &s, int units) {
    const AttnArgs &a = s.p;
    const double keys = (double)units * a.T, rows = (double)units * a.G, wr = a.pk ? 2.0 : 1.0;
    const unsigned chunks = (unsigned)((int64_t)units * s.nchunks);
    {
        ProfScope ps(ctx, "attn_split_scores_kernel", 2.0 * rows * a.T * a.D, 4.0 * wr * keys * a.D + 4.0 * rows * a.T);
        if (a.D == 64) hipLaunchKernelGGL(attn_split_scores_kernel<64>, dim3(chunks), dim3(SPL_THREADS), 0, ctx->stream, s);
        else hipLaunchKernelGGL(attn_split_scores_kernel<128>, dim3(chunks), dim3(SPL_THREADS), 0, ctx->stream, s);
        RTEN_LAUNCH_CHECK(ctx, "attn_split_scores_kernel");
    }
    {
        ProfScope ps(ctx, "attn_split_softmax_kernel", 0.0, 8.0 * rows * a.T);
        hipLaunchKernelGGL(attn_split_softmax_kernel, dim3((unsigned)(units * a.G)), dim3(SM_THREADS), 0, ctx->stream, s);
        RTEN_LAUNCH_CHECK(ctx, "attn_split_softmax_kernel");
    }
    {
        ProfScope ps(ctx, "attn_split_pv_kernel", 2.0 * rows * a.T * a.Dv, 4.0 * wr * keys * a.Dv + 4.0 * rows * a.T + 4.0 * rows * s.NB * a.Dv);
        if (a.Dv == 64) hipLaunchKernelGGL(attn_split_pv_kernel<64>, dim3(chunks), dim3(SPL_THREADS), 0, ctx->stream, s);
        else hipLaunchKernelGGL(attn_split_pv_kernel<128>, dim3(chunks), dim3(SPL_THREADS), 0, ctx->stream, s);
        RTEN_LAUNCH_CHECK(ctx, "attn_split_pv_kernel");
    }
    {
        ProfScope ps(ctx, "attn_split_fold_kernel", 0.0, 4.0 * rows * s.NB * a.Dv + 4.0 * rows * a.Dv);
        hipLaunchKernelGGL(attn_split_fold_kernel, dim3((unsigned)(units * a.G * (a.Dv / FOLD_COLS))), dim3(256), 0, ctx->stream, s);
        RTEN_LAUNCH_CHECK(ctx, "attn_split_fold_kernel");
    }
    return RTEN_HIP_OK;
}

} // namespace

bool rten_attn_split_covers(const AttnArgs &a) { return (a.D == 64 || a.D == 128) && (a.Dv == 64 || a.Dv == 128) && a.G <= PV_TILE / 8; }

// The chunk length when none is set: 16 workgroups per compute unit, between 32 and 1024 keys (docs/KERNELS.md 4.19 has the sweep).
int rten_attn_split_keys(const rten_hip_ctx *ctx, const AttnArgs &a) {
    const int64_t want = 16 * (int64_t)ctx->num_cus;
    const int64_t keys = ((int64_t)a.T * a.B * a.Hkv + want - 1) / want;
    const int64_t ck = (keys + 7) / 8 * 8;
    return (int)(ck < 32 ? 32 : (ck > 1024 ? 1024 : ck));
}

// Mode 0, where the one-workgroup kernel covers the call as well: the split form when B * Hkv workgroups leave most compute units idle and the cache is long
// enough to pay for three more launches (docs/KERNELS.md 4.19 has the measurements; the rule stays inside the measured range).
bool rten_attn_split_pays(const rten_hip_ctx *ctx, const AttnArgs &a) { return (int64_t)a.B * a.Hkv * 8 <= ctx->num_cus && a.T >= 512; }

int32_t rten_attn_split_launch(rten_hip_ctx *ctx, const AttnArgs &a, int keys_per_workgroup) {
    const SplitPlan pl = plan_of(a);
    SplitArgs s = {};
    s.p = a;
    s.ck = keys_per_workgroup > 0 ? keys_per_workgroup : rten_attn_split_keys(ctx, a);
    s.nchunks = (int)(((int64_t)a.T + s.ck - 1) / s.ck);
    s.Tp = pl.Tp;
    s.NB = pl.NB;
    long long cbl = 128;
    if (a.gemv_threads > 0) {
        cbl = ((long long)a.T + a.gemv_threads - 1) / a.gemv_threads;
        if (cbl < 128) cbl = 128;
    }
    s.cb = (int)(cbl > 0x7fffffff ? 0x7fffffff : cbl);
    if ((int64_t)pl.per_pass * s.nchunks > 0x7fffffff || (int64_t)pl.per_pass * a.G * (a.Dv / FOLD_COLS) > 0x7fffffff)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "attention: the split decode form would need more than 2^31 - 1 workgroups in one launch");
    float *aux = (float *)rten_aux_scratch(ctx, (pl.inv_elems + pl.e_elems + pl.bs_elems) * sizeof(float) + 256);
    if (!aux) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "attention: scratch allocation failed (warm up before capture)");
    s.inv = aux + 64;
    s.e = s.inv + pl.inv_elems;
    s.bs = s.e + pl.e_elems;
    for (s.u0 = 0; s.u0 < pl.units; s.u0 += pl.per_pass) {
        const int units = pl.units - s.u0 < pl.per_pass ? pl.units - s.u0 : pl.per_pass;
        const int32_t rc = launch_pass(ctx, s, units);
        if (rc) return rc;
    }
    return RTEN_HIP_OK;
}
