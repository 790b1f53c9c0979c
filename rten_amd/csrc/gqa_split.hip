// GroupQueryAttention decode (S == 1, gemv order on, D 64 / 128) with the key range of one (batch, KV head) spread over many workgroups.  The arithmetic is
// that of gqa_decode_kernel (gqa.hip), order for order, so every split gives the bits of tests/gqa_rules.py; what changes is where a value lives: score rows
// sit in device scratch instead of LDS, so no row has to fit a workgroup, and a batch-1 call fills the device.
//
// Four dependent launches on the stream after gqa_prepare_kernel; no workgroup waits on another, there is no counter and nothing to restore, so a captured
// call replays.  A "unit" is one (batch, KV head); a "chunk" is keys_per_workgroup keys (a multiple of 8, so no 8-key depth block straddles two workgroups).
//   1. gqa_split_scores_kernel<D>, one workgroup of 256 threads per (unit, chunk): the scores of its keys for the G heads of the group, so a K row is
//      fetched once per group.  16 lanes per key, lane l owns depths l + 16 j, folded + 8, + 4, + 2, + 1, then scale * acc; which keys are the left-overs
//      of a column block (scalar fmaf chain, acc * scale) follows the DEVICE kv_len, not the chunk.  Then the window / bias modification.  The query rows
//      are parked in LDS 16 heads at a time (8 KiB whatever G is; a group of more than 16 heads walks its K chunk again out of cache).
//   2. gqa_split_softmax_kernel, one workgroup of 1024 threads per score row: the maximum from f32::MIN (order-free); e = exp_reduced(x - max) for 4096
//      elements at a time, written back over x and into an LDS tile; 16 lanes of wave 0 run the 16 ordered chains over the tile (chain l adds the elements
//      i = l mod 16 in index order) while the other waves fill the second tile; lanes 0..15 added from lane 0; 1 / sum stored per row.  A chain is never
//      split, and its loads come from LDS: T / 16 dependent adds is what this launch costs.
//   3. gqa_split_pv_kernel<D>, one workgroup of 256 threads per (unit, chunk): thread = (output column, block slot).  For each 8-key depth block of the
//      chunk, V is read once and, per head, chained from zero with p = e * (1 / sum), NaN -> 0, which is rounded once per (head, key) into an LDS tile of
//      16 KiB (4096 / G keys at a time) and read from there as a broadcast.  The block sums go to scratch [row, block, D].  Masked keys inside kv_len enter with probability 0; rows at or beyond kv_len
//      are never read.
//   4. gqa_split_fold_kernel, one workgroup of 256 threads per (row, 32 output columns): 128 blocks x 32 columns are staged into LDS with 16-byte loads
//      (the next tile is in flight while this one is folded), and 32 threads fold them in block order: block 0 stored, the rest added left to right.
// Workgroups whose chunk lies at or beyond the device kv_len exit at once; every kernel derives the lengths through lens().  Stages 2 and 4 are device
// functions of split_rows.h, shared with attention_split.hip.
//
// Scratch (floats, after the rotated Q in rten_aux_scratch), a function of host-known dims only.  With Tp = T rounded up to 64 and NB = ceil(T / 8), one
// unit needs G * (Tp + NB * D) floats (score rows, block sums; the block sums cost G / 8 of the V bytes in traffic).  The units are worked through in
// passes of U = clamp(64 MiB / unit bytes, 1, B * KV) units, and the buffer is  round_up(U * G, 64) [1 / sum]  +  U * G * Tp  +  U * G * NB * D.
#include "gqa_common.h"
#include "split_rows.h"

namespace {

constexpr int SPL_THREADS = 256;
constexpr int SPL_QH = 16;       // query heads parked in LDS at a time
constexpr int PV_TILE = 4096;    // probabilities parked in LDS at a time (floats): 8-key blocks of the G heads
constexpr size_t SPLIT_PASS_BYTES = 64u << 20;
constexpr float NEG_INF = -__builtin_inff();

struct SplitArgs {
    GqaArgs p;
    float *inv, *e, *bs; // [U * G], [U * G, Tp], [U * G, NB, D]
    int u0;              // first unit of this pass
    int ck, nchunks, Tp, NB;
};

struct Unit {
    int ul, b, g, kv_len, past_len;
};

__device__ __forceinline__ Unit unit_of(const SplitArgs &s, int ul) {
    Unit u;
    u.ul = ul;
    u.b = (s.u0 + ul) / s.p.KV;
    u.g = (s.u0 + ul) % s.p.KV;
    lens(s.p, u.b, u.kv_len, u.past_len);
    return u;
}

template <int D>
__global__ __launch_bounds__(SPL_THREADS) void gqa_split_scores_kernel(const SplitArgs s) {
    __shared__ float qs[SPL_QH * D];
    const GqaArgs &p = s.p;
    const int tid = threadIdx.x, G = p.G;
    const Unit u = unit_of(s, blockIdx.x / s.nchunks);
    const int64_t t_lo64 = (int64_t)(blockIdx.x % s.nchunks) * s.ck;
    if (t_lo64 >= u.kv_len) return;
    const int t_lo = (int)t_lo64, t_hi = u.kv_len - t_lo < s.ck ? u.kv_len : t_lo + s.ck;
    int start, lim;
    window(p, u.past_len, 0, start, lim);
    long long cbl = 128;
    if (p.gemv_threads > 0) {
        cbl = ((long long)u.kv_len + p.gemv_threads - 1) / p.gemv_threads;
        if (cbl < 128) cbl = 128;
    }
    const int cb = (int)cbl;
    const float *kb = p.pk + ((int64_t)u.b * p.KV + u.g) * p.T * D;
    const int l = tid & 15, grp = tid >> 4;
    for (int h0 = 0; h0 < G; h0 += SPL_QH) {
        const int nh = G - h0 < SPL_QH ? G - h0 : SPL_QH;
        const float *q = p.q + u.b * p.q_sb + ((int64_t)u.g * G + h0) * p.q_sh;
        if (h0) __syncthreads();
        for (int i = tid; i < nh * D; i += SPL_THREADS) qs[i] = q[(i / D) * p.q_sh + (i % D)];
        __syncthreads();
        const float *bias = p.bias ? p.bias + u.b * p.bias_sb + ((int64_t)u.g * G + h0) * p.bias_sh : nullptr;
        float *xr = s.e + ((int64_t)u.ul * G + h0) * s.Tp;
        for (int t0 = t_lo; t0 < t_hi; t0 += SPL_THREADS / 16) {
            const int t = t0 + grp;
            const bool live = t < t_hi;
            const int tt = live ? t : t_hi - 1;
            const int c0 = tt / cb * cb, nc = u.kv_len - c0 < cb ? u.kv_len - c0 : cb;
            const bool vec = (tt - c0) < nc / 8 * 8; // else: a left-over key of its column block -> the scalar chain
            const float *kr = kb + (int64_t)tt * D;
            float kreg[D / 16];
#pragma unroll
            for (int j = 0; j < D / 16; j++) kreg[j] = kr[l + 16 * j];
            const bool inside = t >= start && t < lim;
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
                    if (inside) {
                        if (bias) o = o + bias[h * p.bias_sh + t];
                    } else {
                        o = NEG_INF;
                    }
                    xr[(int64_t)h * s.Tp + t] = o;
                }
            }
        }
    }
}

// stage 2 (split_rows.h) on one score row in scratch: e over x, 1 / sum to inv
__global__ __launch_bounds__(SM_THREADS) void gqa_split_softmax_kernel(const SplitArgs s) {
    const int row = blockIdx.x;
    split_softmax_row(s.e + (int64_t)row * s.Tp, unit_of(s, row / s.p.G).kv_len, s.inv + row);
}

// one 8-key depth block of column n for the G heads: the fmaf chains from zero over `depth` keys, probabilities from LDS (row stride kt)
template <int D, bool FULL>
__device__ __forceinline__ void block_sums(const float *vp, const float *pr, int kt, int depth, int G, float *dst, int64_t dst_stride) {
    float vv[8];
#pragma unroll
    for (int k = 0; k < 8; k++) vv[k] = (FULL || k < depth) ? vp[(int64_t)k * D] : 0.f;
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

template <int D>
__global__ __launch_bounds__(SPL_THREADS) void gqa_split_pv_kernel(const SplitArgs s) {
    constexpr int NS = SPL_THREADS / D; // depth blocks chained side by side
    __shared__ __attribute__((aligned(16))) float ps[PV_TILE];
    const GqaArgs &p = s.p;
    const int tid = threadIdx.x, G = p.G;
    const Unit u = unit_of(s, blockIdx.x / s.nchunks);
    const int64_t t_lo64 = (int64_t)(blockIdx.x % s.nchunks) * s.ck;
    if (t_lo64 >= u.kv_len) return;
    const int t_lo = (int)t_lo64, t_hi = u.kv_len - t_lo < s.ck ? u.kv_len : t_lo + s.ck;
    const int n = tid % D, sl = tid / D;
    const float *vb = p.pv + ((int64_t)u.b * p.KV + u.g) * p.T * D + n;
    const int64_t row0 = (int64_t)u.ul * G;
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
            const int k0 = blk * 8, depth = u.kv_len - k0;
            float *dst = s.bs + (row0 * s.NB + blk) * D + n;
            if (depth >= 8) block_sums<D, true>(vb + (int64_t)k0 * D, ps + (k0 - k_lo), kt, 8, G, dst, (int64_t)s.NB * D);
            else block_sums<D, false>(vb + (int64_t)k0 * D, ps + (k0 - k_lo), kt, depth, G, dst, (int64_t)s.NB * D);
        }
    }
}

// stage 4 (split_rows.h) on 32 output columns of one row
__global__ __launch_bounds__(256) void gqa_split_fold_kernel(const SplitArgs s) {
    const GqaArgs &p = s.p;
    const int D = p.D, slices = D / FOLD_COLS;
    const int row = blockIdx.x / slices, cs = blockIdx.x % slices * FOLD_COLS;
    const Unit u = unit_of(s, row / p.G);
    split_fold_row(s.bs + (int64_t)row * s.NB * D + cs, (u.kv_len + 7) / 8, D, p.out + (int64_t)u.b * p.H * D + ((int64_t)u.g * p.G + row % p.G) * D + cs);
}

struct SplitPlan {
    int Tp, NB, units, per_pass;
    size_t inv_elems, e_elems, bs_elems;
};

SplitPlan plan_of(const GqaArgs &a) {
    SplitPlan pl;
    pl.Tp = (a.T + 63) / 64 * 64;
    pl.NB = (a.T + 7) / 8;
    pl.units = a.B * a.KV;
    const size_t unit_bytes = sizeof(float) * (size_t)a.G * ((size_t)pl.Tp + (size_t)pl.NB * a.D);
    size_t per = SPLIT_PASS_BYTES / unit_bytes;
    per = per < 1 ? 1 : (per > (size_t)pl.units ? (size_t)pl.units : per);
    pl.per_pass = (int)per;
    pl.inv_elems = (per * a.G + 63) / 64 * 64;
    pl.e_elems = per * a.G * pl.Tp;
    pl.bs_elems = per * a.G * (size_t)pl.NB * a.D;
    return pl;
}

template <int D>
int32_t launch_pass(rten_hip_ctx *ctx, const SplitArgs &s, int units) {
    const GqaArgs &a = s.p;
    const double keys = (double)units * a.T, rows = (double)units * a.G;
    const unsigned chunks = (unsigned)((int64_t)units * s.nchunks);
    {
        ProfScope ps(ctx, "gqa_split_scores_kernel", 2.0 * rows * a.T * D, 4.0 * keys * D + 4.0 * rows * a.T);
        hipLaunchKernelGGL(gqa_split_scores_kernel<D>, dim3(chunks), dim3(SPL_THREADS), 0, ctx->stream, s);
        RTEN_LAUNCH_CHECK(ctx, "gqa_split_scores_kernel");
    }
    {
        ProfScope ps(ctx, "gqa_split_softmax_kernel", 0.0, 8.0 * rows * a.T);
        hipLaunchKernelGGL(gqa_split_softmax_kernel, dim3((unsigned)(units * a.G)), dim3(SM_THREADS), 0, ctx->stream, s);
        RTEN_LAUNCH_CHECK(ctx, "gqa_split_softmax_kernel");
    }
    {
        ProfScope ps(ctx, "gqa_split_pv_kernel", 2.0 * rows * a.T * D, 4.0 * keys * D + 4.0 * rows * a.T + 4.0 * rows * s.NB * D);
        hipLaunchKernelGGL(gqa_split_pv_kernel<D>, dim3(chunks), dim3(SPL_THREADS), 0, ctx->stream, s);
        RTEN_LAUNCH_CHECK(ctx, "gqa_split_pv_kernel");
    }
    {
        ProfScope ps(ctx, "gqa_split_fold_kernel", 0.0, 4.0 * rows * s.NB * D + 4.0 * rows * D);
        hipLaunchKernelGGL(gqa_split_fold_kernel, dim3((unsigned)(units * a.G * (D / FOLD_COLS))), dim3(256), 0, ctx->stream, s);
        RTEN_LAUNCH_CHECK(ctx, "gqa_split_fold_kernel");
    }
    return RTEN_HIP_OK;
}

} // namespace

size_t rten_gqa_split_scratch_elems(const GqaArgs &a) {
    const SplitPlan pl = plan_of(a);
    return pl.inv_elems + pl.e_elems + pl.bs_elems;
}

// The chunk length when none is set: 16 workgroups per compute unit (two rounds of the eight that fit), between 32 and 1024 keys (docs/KERNELS.md 4.18 has the sweep).
int rten_gqa_split_keys(const rten_hip_ctx *ctx, const GqaArgs &a) {
    const int64_t want = 16 * (int64_t)ctx->num_cus;
    const int64_t keys = ((int64_t)a.T * a.B * a.KV + want - 1) / want;
    const int64_t ck = (keys + 7) / 8 * 8;
    return (int)(ck < 32 ? 32 : (ck > 1024 ? 1024 : ck));
}

// Mode 0, where the one-workgroup kernel fits as well: the split form when B * KV workgroups leave most compute units idle and the cache is long enough to
// pay for three more launches.  Measured (docs/KERNELS.md 4.18): it wins at 8 and 32 workgroups from 512 keys on and loses at 256; between 32 and 256
// workgroups and below 512 keys nothing was measured, so the rule stays inside the measured range.
bool rten_gqa_split_pays(const rten_hip_ctx *ctx, const GqaArgs &a) { return (int64_t)a.B * a.KV * 8 <= ctx->num_cus && a.T >= 512; }

int32_t rten_gqa_split_launch(rten_hip_ctx *ctx, const GqaArgs &a, int keys_per_workgroup, float *scratch) {
    const SplitPlan pl = plan_of(a);
    SplitArgs s = {};
    s.p = a;
    s.inv = scratch;
    s.e = s.inv + pl.inv_elems;
    s.bs = s.e + pl.e_elems;
    s.ck = keys_per_workgroup > 0 ? keys_per_workgroup : rten_gqa_split_keys(ctx, a);
    s.nchunks = (int)(((int64_t)a.T + s.ck - 1) / s.ck);
    s.Tp = pl.Tp;
    s.NB = pl.NB;
    if (a.G > PV_TILE / 8)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "gqa: the split decode form takes at most %d query heads per KV head", PV_TILE / 8);
    if ((int64_t)pl.per_pass * s.nchunks > 0x7fffffff)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "gqa: the split decode form would need more than 2^31 - 1 workgroups in one launch");
    for (s.u0 = 0; s.u0 < pl.units; s.u0 += pl.per_pass) {
        const int units = pl.units - s.u0 < pl.per_pass ? pl.units - s.u0 : pl.per_pass;
        const int32_t rc = a.D == 64 ? launch_pass<64>(ctx, s, units) : launch_pass<128>(ctx, s, units);
        if (rc) return rc;
    }
    return RTEN_HIP_OK;
}
