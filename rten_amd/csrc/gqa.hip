// GroupQueryAttention with a KV cache: gqa_present_cache and GroupQueryAttention::run_impl, src/ops/attention/contrib.rs:359-878, on sdpa_head
// (src/ops/attention.rs:518-562).
//
//   kv_len(b) = seqlens_k[b] + 1, past_len(b) = 0 when S == total else kv_len(b) - S            (contrib.rs:616,655-661,755)
//   present[b, g] = zeros; rows [0, past_len) <- past[b, g]; rows [past_len, past_len + S) <- the new tokens (K rotated)   (contrib.rs:393-408)
//   out[b, :, h] = softmax(mod(scale * Q[b, h] K[b, h / G, :kv_len]^T)) V[b, h / G, :kv_len],  G = H / KV                      (contrib.rs:741-795)
//   mod, row s: lim = past_len + s + 1; start = lim - local when a window is set and lim > local, else 0; bias added on [start, lim), every other
//   position OVERWRITTEN with -inf (contrib.rs:767-794).
//
// seqlens_k and total are read on the device by every kernel here (lens()), clamped so that no access leaves a buffer: kv_len into [1, P + S], past_len
// into [0, P].  Nothing is read back, so a call captures and a replay follows new device values.
//
// Three kernels:
//   * gqa_prepare_kernel: one launch writes both present caches (zero rows included) and, with rotary, the rotated Q into scratch; K is rotated while it
//     is written.  Rotary is rot1 of decoder.hip: every product and sum rounded on its own; the cache row is gathered as RotaryEmbedding gathers it.
//   * gqa_decode_kernel<D> (S == 1, gemv order on, D 64 / 128): one workgroup of 1024 threads per (batch, KV head) serves the G query heads of the group, so
//     each K and V row leaves HBM once per group instead of G times.  It restates the one-row orders of gemv_f32.hip:
//       - scores, transposed-B form: 16 lanes per key, lane l owns depths l + 16 j (64 contiguous bytes per 16 lanes); 16 lane accumulators over the D / 16
//         depth tiles, folded l + (l + 8), + 4, + 2, + 1, then alpha * acc; the < 8 keys left over in a column block of max(128, ceil(kv_len / threads))
//         keys take the scalar fmaf chain and acc * alpha.  D <= 512 is one depth block, so there is no beta step.
//       - the score modification above, then the three-pass softmax of rowwise.hip (maximum from f32::MIN, ReducedRangeExp, 16 ordered lane sums added from
//         lane 0, e * (1 / sum), NaN -> 0) on the rows in LDS, one wave per head.  Not an online softmax: nothing is rescaled.
//       - PV, row-major-B form: depth blocks of 8 keys, each an fmaf chain from zero; the first block stored, the rest added left to right.  1024 / D
//         blocks are chained in parallel per round (thread = output column x block slot, for up to 8 heads at a time), parked in LDS, and folded in block
//         order by the thread that owns (head, column).  D is 64 or 128: every column lies in a 32-wide tile of its column block (no left-over columns).
//       Masked keys inside kv_len enter the chains with probability 0, as in the reference (a NaN in V there propagates); rows at or beyond kv_len are never
//       read.
//     LDS: 4 * (G * D [q] + 8192 [block sums: 1024 / D slots x 8 heads x D] + G * (P + 1) [score rows]) bytes, which must fit the 160 KiB a single
//     workgroup may declare on this part.  G = 4, D = 128: P + 1 <= 8064 keys.
//   * gqa_scores_kernel: the score modification and softmax for the composed path (GEMM, this kernel, GEMM; the group is the GEMMs' inner batch level with
//     stride 0 on K and V, so nothing is expanded).  It works on all P + S columns: columns at or beyond lim are -inf, contribute exp = 0 to the lane sums
//     and probability 0 to PV, which walks the zero rows of present beyond kv_len: x + 0 and fmaf(0, 0, x) change nothing but the sign of a zero.  The
//     first prompt and a chunk appended to a full cache have kv_len == P + S and are exact.  The query rows are worked through in passes whose score
//     buffer [B, H, rows, P + S] stays within 64 MiB, so scratch does not grow with the square of the prompt.
//   * gqa_row_scores_kernel: one query row on the composed path (other head sizes, rows too long for LDS) in the gemv order.  The first product is NOT the
//     gemv entry on P + 1 columns: which keys are a column block's left-overs follows the DEVICE kv_len, as in the reference, so a right-padded item keeps the
//     reference's bits.  PV is the gemv entry over P + 1 keys; the keys beyond kv_len have probability 0 and zero rows, and a chain that starts at +0
//     cannot be moved by +-0 addends.  (Head sizes above 512 would need the depth-block beta step: refused.)
#include "internal.h"
#include "rowreduce.h"
#include "vecmath.h"

namespace {

struct GqaArgs {
    int B, S, H, KV, D, P, T, G; // T = P + S
    int rot, interleaved, max_pos, local;
    int s0, SC; // composed path: the query rows [s0, s0 + SC) of this pass; scores is [B, H, SC, T]
    long long gemv_threads;
    int64_t q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh, bias_sb, bias_sh, bias_sr;
    const float *q, *k, *v, *past_k, *past_v, *cos, *sin, *bias;
    const int32_t *seqlens, *total, *pos;
    float *qr;       // rotated Q [B, S, H, D] (rotary only)
    float *pk, *pv;  // present [B, KV, T, D]
    float *scores;   // composed path: [B, H, S, T]
    float *out;      // [B, S, H * D]
    float scale;
};

__device__ __forceinline__ void lens(const GqaArgs &p, int b, int &kv_len, int &past_len) {
    long long kv = (long long)p.seqlens[b] + 1;
    kv = kv < 1 ? 1 : (kv > p.T ? p.T : kv);
    long long pl = p.total[0] == p.S ? 0 : kv - p.S;
    pl = pl < 0 ? 0 : (pl > p.P ? p.P : pl);
    kv_len = (int)kv;
    past_len = (int)pl;
}

__device__ __forceinline__ int past_len_of(const GqaArgs &p, int b) {
    int kv_len, past_len;
    lens(p, b, kv_len, past_len);
    return past_len;
}

__device__ __forceinline__ void window(const GqaArgs &p, int past_len, int s, int &start, int &lim) {
    lim = past_len + s + 1;
    start = (p.local > 0 && lim > p.local) ? lim - p.local : 0;
}

// element i of token (b, s), head h of x after rotary (embedding.rs:144-194; rot1 of decoder.hip)
__device__ __forceinline__ float rotated(const GqaArgs &p, const float *xr, int b, int s, int past_len, int i) {
    if (i >= p.rot) return xr[i];
    const int half = p.rot / 2;
    int id = p.pos ? p.pos[(int64_t)b * p.S + s] : past_len + s;
    if (id < 0) id += p.max_pos;
    id = id < 0 ? 0 : (id >= p.max_pos ? p.max_pos - 1 : id);
    int j, i1, i2;
    bool first;
    if (p.interleaved) { j = i >> 1; i1 = 2 * j; i2 = i1 + 1; first = (i & 1) == 0; }
    else { first = i < half; j = first ? i : i - half; i1 = j; i2 = half + j; }
    const float c = p.cos[(int64_t)id * half + j], sn = p.sin[(int64_t)id * half + j];
    const float x1 = xr[i1], x2 = xr[i2];
    return first ? __fsub_rn(__fmul_rn(x1, c), __fmul_rn(x2, sn)) : __fadd_rn(__fmul_rn(x1, sn), __fmul_rn(x2, c));
}

// work items: 2 * B * KV * T * D cache elements, then (rotary) B * S * H * D query elements
__global__ __launch_bounds__(256) void gqa_prepare_kernel(const GqaArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t cache = (int64_t)p.B * p.KV * p.T * p.D;
    if (idx < 2 * cache) {
        const bool is_v = idx >= cache;
        int64_t e = is_v ? idx - cache : idx;
        const int d = (int)(e % p.D);
        e /= p.D;
        const int t = (int)(e % p.T);
        e /= p.T;
        const int g = (int)(e % p.KV), b = (int)(e / p.KV);
        const int past_len = past_len_of(p, b);
        float val = 0.f;
        if (t < past_len) {
            val = (is_v ? p.past_v : p.past_k)[(((int64_t)b * p.KV + g) * p.P + t) * p.D + d];
        } else if (t < past_len + p.S) {
            const int s = t - past_len;
            if (is_v) val = p.v[b * p.v_sb + s * p.v_ss + g * p.v_sh + d];
            else val = rotated(p, p.k + b * p.k_sb + s * p.k_ss + g * p.k_sh, b, s, past_len, d);
        }
        (is_v ? p.pv : p.pk)[idx - (is_v ? cache : 0)] = val;
        return;
    }
    if (!p.qr) return;
    int64_t e = idx - 2 * cache;
    if (e >= (int64_t)p.B * p.S * p.H * p.D) return;
    const int64_t at = e;
    const int d = (int)(e % p.D);
    e /= p.D;
    const int h = (int)(e % p.H);
    e /= p.H;
    const int s = (int)(e % p.S), b = (int)(e / p.S);
    const int past_len = past_len_of(p, b);
    p.qr[at] = rotated(p, p.q + b * p.q_sb + s * p.q_ss + h * p.q_sh, b, s, past_len, d);
}

constexpr int DEC_THREADS = 1024;
constexpr int DEC_HC = 8; // heads whose block sums are parked at a time
constexpr float NEG_INF = -__builtin_inff();

// the softmax of rowwise.hip (softmax_long_kernel) on a row one wave owns, in place
__device__ __forceinline__ void softmax_row(float *row, int cols, int lane) {
    float mx = -3.40282347e+38f; // f32::MIN (softmax.rs:181)
    for (int i = lane; i < cols; i += 64) mx = fmaxf(mx, row[i]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float a = 0.f;
    const int l = lane & 15;
    const int nch = (cols + 63) / 64;
    for (int c = 0; c < nch; c++) {
        const int i = c * 64 + lane;
        float e = 0.f;
        if (i < cols) {
            e = vm::exp_reduced(row[i] - mx);
            row[i] = e;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float eq = lane_bcast(e, l + 16 * q);
            if (c * 64 + l + 16 * q < cols) a = a + eq;
        }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k++) s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), k));
    const float inv = 1.0f / s;
    for (int i = lane; i < cols; i += 64) {
        float r = row[i] * inv;
        if (!(r == r)) r = 0.f; // flush_nans_to_zero (attention.rs:551)
        row[i] = r;
    }
}

template <int D>
__global__ __launch_bounds__(DEC_THREADS) void gqa_decode_kernel(const GqaArgs p) {
    extern __shared__ float smem[];
    constexpr int NS = DEC_THREADS / D; // depth blocks chained per round
    const int G = p.G, T = p.T;
    float *qs = smem;                       // [G][D]
    float *bs = qs + G * D;                 // [NS][DEC_HC][D]
    float *sc = bs + DEC_THREADS * DEC_HC;  // [G][T]
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    int kv_len, past_len, start, lim;
    lens(p, b, kv_len, past_len);
    window(p, past_len, 0, start, lim);
    const float *q = p.q + b * p.q_sb + (int64_t)g * G * p.q_sh;
    for (int i = tid; i < G * D; i += DEC_THREADS) qs[i] = q[(i / D) * p.q_sh + (i % D)];
    __syncthreads();

    // ---- scores: 16 lanes per key, 64 keys per pass
    long long cbl = 128;
    if (p.gemv_threads > 0) {
        cbl = ((long long)kv_len + p.gemv_threads - 1) / p.gemv_threads;
        if (cbl < 128) cbl = 128;
    }
    const int cb = (int)cbl;
    const float *kb = p.pk + ((int64_t)b * p.KV + g) * T * D;
    const float *bias = p.bias ? p.bias + b * p.bias_sb + (int64_t)g * G * p.bias_sh : nullptr;
    const int l = tid & 15, grp = tid >> 4;
    for (int t0 = 0; t0 < kv_len; t0 += DEC_THREADS / 16) {
        const int t = t0 + grp;
        const bool live = t < kv_len;
        const int tt = live ? t : kv_len - 1;
        const int c0 = tt / cb * cb, nc = kv_len - c0 < cb ? kv_len - c0 : cb;
        const bool vec = (tt - c0) < nc / 8 * 8; // else: a left-over key of its column block -> the scalar chain
        const float *kr = kb + (int64_t)tt * D;
        float kreg[D / 16];
#pragma unroll
        for (int j = 0; j < D / 16; j++) kreg[j] = kr[l + 16 * j];
        const bool inside = t >= start && t < lim;
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
                if (inside) {
                    if (bias) o = o + bias[h * p.bias_sh + t];
                } else {
                    o = NEG_INF;
                }
                sc[h * T + t] = o;
            }
        }
    }
    __syncthreads();

    // ---- softmax: one wave per head
    for (int h = tid >> 6; h < G; h += DEC_THREADS / 64) softmax_row(sc + h * T, kv_len, tid & 63);
    __syncthreads();

    // ---- PV: thread = (column n, block slot sl); the owner of (head hh, column nn) folds the parked block sums in block order
    const int n = tid % D, sl = tid / D;
    const int hh_own = tid / D, nn_own = tid % D; // (DEC_HC * D <= DEC_THREADS)
    const float *vb = p.pv + ((int64_t)b * p.KV + g) * T * D;
    const int nblk = (kv_len + 7) / 8;
    float *outb = p.out + (int64_t)b * p.H * D + (int64_t)g * G * D;
    for (int hc0 = 0; hc0 < G; hc0 += DEC_HC) {
        const int nh = G - hc0 < DEC_HC ? G - hc0 : DEC_HC;
        const bool owner = hh_own < nh;
        float o = 0.f;
        for (int blk0 = 0; blk0 < nblk; blk0 += NS) {
            const int blk = blk0 + sl;
            float acc[DEC_HC];
#pragma unroll
            for (int hh = 0; hh < DEC_HC; hh++) acc[hh] = 0.f;
            if (blk < nblk) {
                const int k0 = blk * 8;
                const int depth = kv_len - k0 < 8 ? kv_len - k0 : 8;
                float vv[8];
#pragma unroll
                for (int k = 0; k < 8; k++) vv[k] = k < depth ? vb[(int64_t)(k0 + k) * D + n] : 0.f;
#pragma unroll
                for (int hh = 0; hh < DEC_HC; hh++) {
                    if (hh < nh) {
                        const float *pr = sc + (hc0 + hh) * T + k0;
#pragma unroll
                        for (int k = 0; k < 8; k++)
                            if (k < depth) acc[hh] = fmaf(pr[k], vv[k], acc[hh]);
                    }
                }
            }
#pragma unroll
            for (int hh = 0; hh < DEC_HC; hh++) bs[(sl * DEC_HC + hh) * D + n] = acc[hh];
            __syncthreads();
            if (owner) {
                const int cnt = nblk - blk0 < NS ? nblk - blk0 : NS;
                for (int s2 = 0; s2 < cnt; s2++) {
                    const float v = bs[(s2 * DEC_HC + hh_own) * D + nn_own];
                    o = (blk0 + s2 == 0) ? v : o + v; // the first block is stored, the rest are added
                }
            }
            __syncthreads();
        }
        if (owner) outb[(hc0 + hh_own) * D + nn_own] = o;
    }
}

// composed path, one query row in the gemv order: scores[b, h, t] = scale * q[b, h] . K[b, h / G, t] for t < kv_len in the transposed-B form of gemv_f32.hip
// (gemv_transposed_kernel), with the column blocks taken from the DEVICE kv_len -- the reference's product has kv_len columns, and which keys are a block's
// left-overs follows from that count.  16 lanes per key; D <= 512 is one depth block.  Keys at or beyond kv_len are left to gqa_scores_kernel (-inf).
__global__ __launch_bounds__(256) void gqa_row_scores_kernel(const GqaArgs p) {
    const int l = threadIdx.x & 15;
    const int t = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int bh = blockIdx.y, h = bh % p.H, b = bh / p.H;
    int kv_len, past_len;
    lens(p, b, kv_len, past_len);
    const bool live = t < kv_len;
    const int tt = live ? t : kv_len - 1;
    long long cbl = 128;
    if (p.gemv_threads > 0) {
        cbl = ((long long)kv_len + p.gemv_threads - 1) / p.gemv_threads;
        if (cbl < 128) cbl = 128;
    }
    const int cb = (int)cbl;
    const int c0 = tt / cb * cb, nc = kv_len - c0 < cb ? kv_len - c0 : cb;
    const bool vec = (tt - c0) < nc / 8 * 8;
    const float *qh = p.q + b * p.q_sb + h * p.q_sh;
    const float *kr = p.pk + (((int64_t)b * p.KV + h / p.G) * p.T + tt) * p.D;
    const int dt = p.D / 16 * 16;
    float part = 0.f;
    for (int d = 0; d < dt; d += 16) part = fmaf(qh[d + l], kr[d + l], part);
    part = part + __shfl_down(part, 8, 16);
    part = part + __shfl_down(part, 4, 16);
    part = part + __shfl_down(part, 2, 16);
    part = part + __shfl_down(part, 1, 16);
    if (!live || l != 0) return;
    float o;
    if (vec) {
        float acc = part;
        for (int k = dt; k < p.D; k++) acc = fmaf(qh[k], kr[k], acc);
        o = p.scale * acc;
    } else {
        float acc = 0.f;
        for (int k = 0; k < p.D; k++) acc = fmaf(qh[k], kr[k], acc);
        o = acc * p.scale;
    }
    p.scores[(int64_t)bh * p.T + t] = o;
}

// composed path: score modification + softmax on row (b, h, s0 + i) of this pass's scores [B, H, SC, T], one wave per row
__global__ __launch_bounds__(256) void gqa_scores_kernel(const GqaArgs p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)p.B * p.H * p.SC) return;
    const int s = p.s0 + (int)(row % p.SC);
    const int64_t bh = row / p.SC;
    const int h = (int)(bh % p.H), b = (int)(bh / p.H);
    int kv_len, past_len, start, lim;
    lens(p, b, kv_len, past_len);
    window(p, past_len, s, start, lim);
    float *r = p.scores + row * p.T;
    const float *bias = p.bias ? p.bias + b * p.bias_sb + h * p.bias_sh + s * p.bias_sr : nullptr;
    for (int i = lane; i < p.T; i += 64) {
        float o = NEG_INF;
        if (i >= start && i < lim) {
            o = r[i];
            if (bias) o = o + bias[i];
        }
        r[i] = o;
    }
    softmax_row(r, p.T, lane);
}

size_t decode_lds_bytes(int G, int D, int T) { return sizeof(float) * ((size_t)G * D + (size_t)DEC_THREADS * DEC_HC + (size_t)G * T); }
constexpr size_t LDS_PER_WORKGROUP = 160 * 1024;
constexpr size_t SCORE_PASS_BYTES = 64u << 20; // the composed path's score buffer per pass over the query rows

template <int D>
int32_t launch_decode(rten_hip_ctx *ctx, const GqaArgs &a, size_t lds) {
    // the kernel's dynamic LDS ceiling, raised once per device (not a stream operation: nothing lands in a capture)
    static std::once_flag raised[64];
    static hipError_t raised_rc[64];
    const int dev = ctx->device & 63;
    std::call_once(raised[dev], [&] {
        raised_rc[dev] = hipFuncSetAttribute((const void *)gqa_decode_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_PER_WORKGROUP);
    });
    RTEN_HIP_TRY(ctx, raised_rc[dev]);
    const double kvb = 8.0 * a.B * a.KV * (double)a.T * D;
    ProfScope ps(ctx, "gqa_decode_kernel", 4.0 * a.B * a.H * (double)a.T * D, kvb + 8.0 * a.B * a.H * D);
    hipLaunchKernelGGL(gqa_decode_kernel<D>, dim3((unsigned)a.KV, (unsigned)a.B), dim3(DEC_THREADS), lds, ctx->stream, a);
    RTEN_LAUNCH_CHECK(ctx, "gqa_decode_kernel");
    return RTEN_HIP_OK;
}

} // namespace

RTEN_EXPORT int32_t rten_hip_set_gqa_path(rten_hip_ctx *ctx, int32_t mode) {
    RTEN_CHECK_CTX(ctx);
    if (mode < 0 || mode > 2) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "set_gqa_path: mode must be 0, 1 or 2");
    ctx->gqa_path = mode;
    return RTEN_HIP_OK;
}

RTEN_EXPORT int32_t rten_hip_gqa_f32(rten_hip_ctx *ctx, const int32_t *dims, const int64_t *strides, float scale, const float *q, const float *k,
                                     const float *v, const float *past_key, const float *past_value, const int32_t *seqlens_k,
                                     const int32_t *total_sequence_length, const float *cos, const float *sin, const int32_t *position_ids,
                                     const float *attention_bias, float *out, float *present_key, float *present_value) {
    RTEN_CHECK_CTX(ctx);
    if (!dims || !strides) return RTEN_HIP_ERR_INVALID_VALUE;
    GqaArgs a = {};
    a.B = dims[0]; a.S = dims[1]; a.H = dims[2]; a.KV = dims[3]; a.D = dims[4]; a.P = dims[5];
    a.rot = dims[6]; a.interleaved = dims[7] != 0; a.max_pos = dims[8]; a.local = dims[9];
    if (a.B < 0 || a.S < 0 || a.H <= 0 || a.KV <= 0 || a.D < 0 || a.P < 0 || a.H % a.KV != 0) return RTEN_HIP_ERR_INVALID_VALUE;
    if (a.rot < 0 || a.rot % 2 != 0 || a.rot > a.D) return RTEN_HIP_ERR_INVALID_VALUE;
    if ((int64_t)a.P + a.S > 0x7fffffff) return RTEN_HIP_ERR_INVALID_VALUE;
    a.T = a.P + a.S; a.G = a.H / a.KV;
    if (a.B == 0 || a.S == 0 || a.D == 0) return RTEN_HIP_OK;
    if (!q || !k || !v || !seqlens_k || !total_sequence_length || !out || !present_key || !present_value) return RTEN_HIP_ERR_INVALID_VALUE;
    if (a.P > 0 && (!past_key || !past_value)) return RTEN_HIP_ERR_INVALID_VALUE;
    if (a.rot > 0 && (!cos || !sin || a.max_pos <= 0)) return RTEN_HIP_ERR_INVALID_VALUE;
    a.q_sb = strides[0]; a.q_ss = strides[1]; a.q_sh = strides[2];
    a.k_sb = strides[3]; a.k_ss = strides[4]; a.k_sh = strides[5];
    a.v_sb = strides[6]; a.v_ss = strides[7]; a.v_sh = strides[8];
    a.bias_sb = strides[9]; a.bias_sh = strides[10]; a.bias_sr = strides[11];
    a.q = q; a.k = k; a.v = v; a.past_k = past_key; a.past_v = past_value; a.cos = cos; a.sin = sin; a.bias = attention_bias;
    a.seqlens = seqlens_k; a.total = total_sequence_length; a.pos = a.rot > 0 ? position_ids : nullptr;
    a.pk = present_key; a.pv = present_value; a.out = out; a.scale = scale;
    a.gemv_threads = ctx->gemv_threads;

    const bool one_row = a.S == 1 && ctx->gemv_order != 0;
    if (one_row && a.D > 512)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "gqa: one query row in the gemv order with a head size above 512 is not supported (one depth block only)");
    const size_t lds = decode_lds_bytes(a.G, a.D, a.T);
    const bool covered = one_row && (a.D == 64 || a.D == 128) && lds <= LDS_PER_WORKGROUP;
    if (ctx->gqa_path == 2 && !covered)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "gqa: the decode kernel takes one query row in the gemv order, head size 64 or 128 and rows that fit LDS");
    const bool fused = covered && ctx->gqa_path != 1;

    // scratch: [rotated Q | scores], the auxiliary buffer (the GEMMs called below own `scratch`).  The composed path works through the query rows in passes
    // of SC rows so that the score buffer [B, H, SC, T] stays within SCORE_PASS_BYTES whatever the prompt length (rows are independent of one another).
    const size_t q_elems = a.rot > 0 ? (size_t)a.B * a.S * a.H * a.D : 0;
    const size_t q_pad = (q_elems + 63) / 64 * 64;
    const size_t row_elems = (size_t)a.B * a.H * (size_t)a.T; // one query row of every (batch, head)
    size_t sc_rows = SCORE_PASS_BYTES / sizeof(float) / row_elems;
    sc_rows = sc_rows < 1 ? 1 : (sc_rows > (size_t)a.S ? (size_t)a.S : sc_rows);
    a.SC = (int)sc_rows;
    const size_t score_elems = fused ? 0 : row_elems * sc_rows;
    float *aux = nullptr;
    if (q_pad + score_elems > 0) {
        aux = (float *)rten_aux_scratch(ctx, (q_pad + score_elems) * sizeof(float) + 256);
        if (!aux) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "gqa: scratch allocation failed (warm up before capture)");
        aux += 64;
    }
    a.qr = q_elems ? aux : nullptr;
    a.scores = score_elems ? aux + q_pad : nullptr;
    {
        const int64_t items = 2 * (int64_t)a.B * a.KV * a.T * a.D + (int64_t)q_elems;
        ProfScope ps(ctx, "gqa_prepare_kernel", 0.0, 4.0 * (double)items * 2);
        hipLaunchKernelGGL(gqa_prepare_kernel, dim3((unsigned)ceil_div64(items, 256)), dim3(256), 0, ctx->stream, a);
        RTEN_LAUNCH_CHECK(ctx, "gqa_prepare_kernel");
    }
    if (a.qr) { // the attention below reads the rotated copy
        a.q = a.qr;
        a.q_sb = (int64_t)a.S * a.H * a.D; a.q_ss = (int64_t)a.H * a.D; a.q_sh = a.D;
    }
    if (fused) return a.D == 64 ? launch_decode<64>(ctx, a, lds) : launch_decode<128>(ctx, a, lds);

    // ---- composed path.  Batch levels: outer = (b, KV head), inner = the G query heads of the group, K and V with inner stride 0.  (b, KV head) is
    // one stride of Q and out only for one batch item, or one token whose batch stride is H heads; otherwise one launch per batch item.
    const bool merged = a.B == 1 || (a.S == 1 && a.q_sb == (int64_t)a.H * a.q_sh);
    const int launches = merged ? 1 : a.B;
    const int outer = merged ? a.B * a.KV : a.KV;
    const int64_t cache_b = (int64_t)a.KV * a.T * a.D, out_b = (int64_t)a.S * a.H * a.D;
    auto gemm = [&](const rten_hip_gemm_desc &g, const float *x, const float *y, float *z) {
        return one_row ? rten_hip_gemm_f32(ctx, &g, x, y, nullptr, z) : rten_gemm_f32_blocked(ctx, &g, x, y, nullptr, z);
    };
    for (a.s0 = 0; a.s0 < a.S; a.s0 += a.SC) {
        if (a.S - a.s0 < a.SC) a.SC = a.S - a.s0;
        const int64_t score_b = (int64_t)a.H * a.SC * a.T;
        if (one_row) { // scores = scale * q K^T over the device kv_len, in the gemv order
            ProfScope ps(ctx, "gqa_row_scores_kernel", 2.0 * a.B * a.H * (double)a.T * a.D, 4.0 * a.B * a.KV * (double)a.T * a.D);
            hipLaunchKernelGGL(gqa_row_scores_kernel, dim3((unsigned)((a.T + 15) / 16), (unsigned)(a.B * a.H)), dim3(256), 0, ctx->stream, a);
            RTEN_LAUNCH_CHECK(ctx, "gqa_row_scores_kernel");
        } else {
            for (int i = 0; i < launches; i++) { // scores = scale * Q K^T
                rten_hip_gemm_desc g = {};
                g.m = a.SC; g.n = a.T; g.k = a.D;
                g.a_rs = a.q_ss; g.a_cs = 1; g.b_rs = 1; g.b_cs = a.D; g.ldc = a.T;
                g.batch = outer * a.G; g.batch_inner = a.G;
                g.a_bs = (int64_t)a.G * a.q_sh; g.a_bsi = a.q_sh;
                g.b_bs = (int64_t)a.T * a.D; g.b_bsi = 0;
                g.c_bs = (int64_t)a.G * a.SC * a.T; g.c_bsi = (int64_t)a.SC * a.T;
                g.alpha = a.scale; g.beta = 0.f;
                const int32_t rc = gemm(g, a.q + i * a.q_sb + a.s0 * a.q_ss, a.pk + i * cache_b, a.scores + i * score_b);
                if (rc) return rc;
            }
        }
        {
            const int64_t rows = (int64_t)a.B * a.H * a.SC;
            ProfScope ps(ctx, "gqa_scores_kernel", 0.0, 8.0 * rows * a.T);
            hipLaunchKernelGGL(gqa_scores_kernel, dim3((unsigned)ceil_div64(rows, 4)), dim3(256), 0, ctx->stream, a);
            RTEN_LAUNCH_CHECK(ctx, "gqa_scores_kernel");
        }
        for (int i = 0; i < launches; i++) { // out = P V
            rten_hip_gemm_desc g = {};
            g.m = a.SC; g.n = a.D; g.k = a.T;
            g.a_rs = a.T; g.a_cs = 1; g.b_rs = a.D; g.b_cs = 1; g.ldc = (int64_t)a.H * a.D;
            g.batch = outer * a.G; g.batch_inner = a.G;
            g.a_bs = (int64_t)a.G * a.SC * a.T; g.a_bsi = (int64_t)a.SC * a.T;
            g.b_bs = (int64_t)a.T * a.D; g.b_bsi = 0;
            g.c_bs = (int64_t)a.G * a.D; g.c_bsi = a.D;
            g.alpha = 1.f; g.beta = 0.f;
            const int32_t rc = gemm(g, a.scores + i * score_b, a.pv + i * cache_b, a.out + i * out_b + (int64_t)a.s0 * a.H * a.D);
            if (rc) return rc;
        }
    }
    return RTEN_HIP_OK;
}
