// The per-token operators of a decoder block around its projections: RMSNormalization / SimplifiedLayerNormalization, the skip forms
// (Skip[Simplified]LayerNormalization) and RotaryEmbedding.  Replaces src/ops/norm.rs:103-161,419-529,571-608, src/ops/norm/contrib.rs:22-77,
// rten-vecmath/src/normalize.rs:112-166, sum.rs:12-34,100-130 and src/ops/embedding.rs:46-207, src/ops/embedding/contrib.rs:32-126.
//
// Normalisation.  The statistic is the reference's fold_unroll<4> over 16-lane vectors (rowreduce.h): 64 independent FMA chains, which are one wave's 64
// lanes, every step one contiguous 256-byte read.  The chains cannot be split over waves without changing the bits, but everything around them can: the
// rows here are 2048-8192 columns wide and in decode there are 1-32 of them, so a WORKGROUP owns a row.  All of its waves load the row (16 bytes per lane),
// form input + skip + bias, park the sum in LDS (and store sum_out), ONE wave folds the statistic out of LDS, and all waves scale their own registers and
// store.  HBM sees every element once.  Rows of at most 1024 columns take the same kernel with one wave per row and four rows per workgroup; rows above
// 8192 columns take a wave-per-row two-pass form that re-reads its operands.
//
// RotaryEmbedding.  One thread per four rotated pairs (two 16-byte loads of x, one each of cos and sin, two 16-byte stores) or per four copied elements;
// a scalar form of the same walk where head size, strides or alignment rule the 16-byte accesses out.  Products and sums are rounded separately as the
// reference's are (this file is built with -ffp-contract=off like every other; the intrinsics below say so where it matters).
#include "internal.h"
#include "rowreduce.h" // simd16_reduce: the reduction order, shared with rowwise.hip and norm.hip
#include "vecmath.h"

namespace {

constexpr int NORM_THREADS = 256;
constexpr int NORM_MAX_COLS = 8192; // one row in LDS: 32 KiB, five workgroups per compute unit

struct NormArgs {
    int64_t rows, skip_rows;
    int cols, vec; // vec: cols % 4 == 0 and every operand 16-byte aligned -> 16-byte accesses
    const float *x, *skip, *bias, *gamma, *beta;
    float gamma_scalar, eps;
    float *sum_out, *y;
};

// Four consecutive elements starting at i (i % 4 == 0): one 16-byte access in the vector form, up to four guarded 4-byte ones otherwise.
__device__ __forceinline__ float4 ld4(const float *__restrict__ p, int i, int n, bool vec, float fill) {
    float4 r = make_float4(fill, fill, fill, fill);
    if (vec) {
        if (i < n) r = *reinterpret_cast<const float4 *>(p + i);
    } else {
        if (i < n) r.x = p[i];
        if (i + 1 < n) r.y = p[i + 1];
        if (i + 2 < n) r.z = p[i + 2];
        if (i + 3 < n) r.w = p[i + 3];
    }
    return r;
}
__device__ __forceinline__ void st4(float *__restrict__ p, int i, int n, bool vec, const float4 v) {
    if (vec) {
        if (i < n) *reinterpret_cast<float4 *>(p + i) = v;
    } else {
        if (i < n) p[i] = v.x;
        if (i + 1 < n) p[i + 1] = v.y;
        if (i + 2 < n) p[i + 2] = v.z;
        if (i + 3 < n) p[i + 3] = v.w;
    }
}
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// The three Normalize forms (normalize.rs:112-166) on one element: FORM 0 = one-element scale, no bias: mul_add(x - m, r, 0) (a -0 product comes out +0);
// FORM 1 = per-element scale only: (x - m) * (g * r); FORM 2 = per-element scale and bias: mul_add(x - m, g * r, b + 0).
template <int FORM>
__device__ __forceinline__ float norm1(float x, float m, float r, float g, float b) {
    if constexpr (FORM == 0) return vm::fma(x - m, r, 0.f);
    else if constexpr (FORM == 1) return (x - m) * (g * r);
    else return vm::fma(x - m, g * r, b + 0.f);
}
template <int FORM>
__device__ __forceinline__ float4 norm4(const float4 x, float m, float r, const float4 g, const float4 b) {
    return make_float4(norm1<FORM>(x.x, m, r, g.x, b.x), norm1<FORM>(x.y, m, r, g.y, b.y), norm1<FORM>(x.z, m, r, g.z, b.z), norm1<FORM>(x.w, m, r, g.w, b.w));
}

// WPR waves per row (1: four rows per workgroup, 4: one), VEC 16-byte groups per thread: covers cols <= WPR * 64 * 4 * VEC.  LN: mean-centred (Sum, then
// SumSquareSub) instead of the root mean square.  y / sum_out may alias x or skip: every wave of a row has read all it needs before the barrier, and stores
// come after it.
template <int WPR, int VEC, bool LN>
__global__ __launch_bounds__(NORM_THREADS) void skip_norm_kernel(const NormArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[]; // rows_per_block rows of cols_pad floats, then {mean, ssr} per row
    constexpr int RPB = 4 / WPR, T = WPR * 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = wave / WPR, t = (wave % WPR) * 64 + lane;
    const int cols = p.cols, cols_pad = (cols + 3) & ~3;
    const int64_t row_raw = (int64_t)blockIdx.x * RPB + slot;
    const bool live = row_raw < p.rows;
    const int64_t row = live ? row_raw : p.rows - 1; // (clamped, not returned: every wave meets the barriers)
    const bool vec = p.vec != 0;
    const float *xr = p.x + row * cols;
    const float *sr = p.skip ? p.skip + (row % p.skip_rows) * cols : nullptr;
    float *row_lds = lds + (size_t)slot * cols_pad;
    float *stat = lds + (size_t)RPB * cols_pad + 2 * slot;

    // everything the row needs is requested here, together: scale and bias depend on nothing, and behind the ordered fold their L2 round trip would be the
    // tail of every workgroup (the comment in layer_norm_kernel, rowwise.hip)
    float4 v[VEC], sv[VEC], bv[VEC], gv[VEC], ev[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) v[k] = ld4(xr, (k * T + t) * 4, cols, vec, 0.f);
    if (sr) {
#pragma unroll
        for (int k = 0; k < VEC; k++) sv[k] = ld4(sr, (k * T + t) * 4, cols, vec, 0.f);
    }
    if (p.bias) {
#pragma unroll
        for (int k = 0; k < VEC; k++) bv[k] = ld4(p.bias, (k * T + t) * 4, cols, vec, 0.f);
    }
#pragma unroll
    for (int k = 0; k < VEC; k++) { gv[k] = make_float4(1.f, 1.f, 1.f, 1.f); ev[k] = make_float4(0.f, 0.f, 0.f, 0.f); }
    if (p.gamma) {
#pragma unroll
        for (int k = 0; k < VEC; k++) gv[k] = ld4(p.gamma, (k * T + t) * 4, cols, vec, 1.f);
    }
    if (LN && p.beta) {
#pragma unroll
        for (int k = 0; k < VEC; k++) ev[k] = ld4(p.beta, (k * T + t) * 4, cols, vec, 0.f);
    }
    // sum = (input + skip) + bias: two separately rounded adds (contrib.rs:52-55)
    if (sr) {
#pragma unroll
        for (int k = 0; k < VEC; k++) v[k] = add4(v[k], sv[k]);
    }
    if (p.bias) {
#pragma unroll
        for (int k = 0; k < VEC; k++) v[k] = add4(v[k], bv[k]);
    }
#pragma unroll
    for (int k = 0; k < VEC; k++) {
        const int i = (k * T + t) * 4;
        if (i < cols) *reinterpret_cast<float4 *>(row_lds + i) = v[k]; // (cols_pad is a multiple of 4: the padding lanes of the last group are never read)
    }
    __syncthreads();
    if (p.sum_out && live) {
        float *so = p.sum_out + row * cols;
#pragma unroll
        for (int k = 0; k < VEC; k++) st4(so, (k * T + t) * 4, cols, vec, v[k]);
    }
    if (wave % WPR == 0) {
        auto get = [&](int i) -> float { return row_lds[i]; };
        float mean = 0.f, var;
        if constexpr (LN) {
            mean = simd16_reduce<0, 8>(get, cols, 0.f, lane) / (float)cols;
            var = simd16_reduce<1, 8>(get, cols, mean, lane) / (float)cols;
        } else {
            var = simd16_reduce<1, 8>(get, cols, 0.f, lane) / (float)cols; // SumSquare: mul_add(x, x, acc) (x - 0 is x)
        }
        if (lane == 0) { stat[0] = mean; stat[1] = p.gamma_scalar / sqrtf(var + p.eps); }
    }
    __syncthreads();
    const float mean = stat[0], ssr = stat[1];
    if (!live) return;
    float *yr = p.y + row * cols;
    const int form = !p.gamma ? 0 : ((LN && p.beta) ? 2 : 1);
    if (form == 0) {
#pragma unroll
        for (int k = 0; k < VEC; k++) st4(yr, (k * T + t) * 4, cols, vec, norm4<0>(v[k], mean, ssr, gv[k], ev[k]));
    } else if (form == 1) {
#pragma unroll
        for (int k = 0; k < VEC; k++) st4(yr, (k * T + t) * 4, cols, vec, norm4<1>(v[k], mean, ssr, gv[k], ev[k]));
    } else {
#pragma unroll
        for (int k = 0; k < VEC; k++) st4(yr, (k * T + t) * 4, cols, vec, norm4<2>(v[k], mean, ssr, gv[k], ev[k]));
    }
}

// Rows above NORM_MAX_COLS columns: one wave per row, two passes over the operands (the second one is served from L2 for any row a decoder has).  The sum
// is re-formed with the same two adds, so both passes see the same bits.  No aliasing of outputs with inputs here.
template <bool LN>
__global__ __launch_bounds__(NORM_THREADS) void skip_norm_stream_kernel(const NormArgs p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (NORM_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const int cols = p.cols;
    const float *xr = p.x + row * cols;
    const float *sr = p.skip ? p.skip + (row % p.skip_rows) * cols : nullptr;
    const float *bias = p.bias;
    auto get = [&](int i) -> float {
        float s = xr[i];
        if (sr) s = s + sr[i];
        if (bias) s = s + bias[i];
        return s;
    };
    float mean = 0.f, var;
    if constexpr (LN) {
        mean = simd16_reduce<0, 8>(get, cols, 0.f, lane) / (float)cols;
        var = simd16_reduce<1, 8>(get, cols, mean, lane) / (float)cols;
    } else {
        var = simd16_reduce<1, 8>(get, cols, 0.f, lane) / (float)cols;
    }
    const float ssr = p.gamma_scalar / sqrtf(var + p.eps);
    float *yr = p.y + row * cols;
    float *so = p.sum_out ? p.sum_out + row * cols : nullptr;
    const int form = !p.gamma ? 0 : ((LN && p.beta) ? 2 : 1);
    for (int i = lane; i < cols; i += 64) {
        const float s = get(i);
        if (so) so[i] = s;
        const float g = p.gamma ? p.gamma[i] : 1.f, b = (LN && p.beta) ? p.beta[i] : 0.f;
        yr[i] = form == 0 ? norm1<0>(s, mean, ssr, g, b) : (form == 1 ? norm1<1>(s, mean, ssr, g, b) : norm1<2>(s, mean, ssr, g, b));
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int32_t skip_norm_launch(rten_hip_ctx *ctx, const char *name, bool ln, NormArgs a) {
    RTEN_CHECK_CTX(ctx);
    if (a.rows < 0 || a.cols < 0) return RTEN_HIP_ERR_INVALID_VALUE;
    if (a.rows == 0 || a.cols == 0) return RTEN_HIP_OK;
    if (!a.x || !a.y) return RTEN_HIP_ERR_INVALID_VALUE;
    if (a.skip && a.skip_rows <= 0) return RTEN_HIP_ERR_INVALID_VALUE;
    if (!a.skip) a.skip_rows = 1;
    a.vec = a.cols % 4 == 0 && aligned16(a.x) && aligned16(a.y) && aligned16(a.skip) && aligned16(a.bias) && aligned16(a.gamma) && aligned16(a.beta) &&
            aligned16(a.sum_out);
    const int cols = a.cols;
    const double words = (double)a.rows * cols * (2 + (a.skip ? 1 : 0) + (a.sum_out ? 1 : 0));
    ProfScope ps(ctx, name, 0.0, 4.0 * words);
    // Launch rule.  One wave per row up to 1024 columns (the register-resident reach of layer_norm_kernel, and a row of that size is one or two 16-byte
    // loads per lane: nothing to spread); a workgroup per row from there to 8192 columns, whatever the row count -- see KERNELS.md 4.17 for the rows behind
    // it; the two-pass form above that.  VEC is the smallest instantiation that covers the row: unused 16-byte groups cost registers, not traffic.
    static const int env_wpr = getenv("RTEN_NORM_WPR") ? atoi(getenv("RTEN_NORM_WPR")) : 0; // (tuning: 1 / 4 force the waves per row where the form covers the row)
    const dim3 block(NORM_THREADS);
    if (cols > NORM_MAX_COLS) {
        const dim3 grid((unsigned)ceil_div64(a.rows, NORM_THREADS / 64));
        if (ln) hipLaunchKernelGGL(skip_norm_stream_kernel<true>, grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL(skip_norm_stream_kernel<false>, grid, block, 0, ctx->stream, a);
        RTEN_LAUNCH_CHECK(ctx, "skip_norm_stream_kernel");
        return RTEN_HIP_OK;
    }
    const bool wide = env_wpr == 4 ? true : (env_wpr == 1 && cols <= 1024 ? false : cols > 1024);
    const int rpb = wide ? 1 : 4;
    const size_t dyn = ((size_t)rpb * ((cols + 3) & ~3) + 2 * rpb) * sizeof(float);
    const dim3 grid((unsigned)ceil_div64(a.rows, rpb));
#define SN_LAUNCH(WPR, VEC) do { if (ln) hipLaunchKernelGGL((skip_norm_kernel<WPR, VEC, true>), grid, block, dyn, ctx->stream, a); \
                                 else hipLaunchKernelGGL((skip_norm_kernel<WPR, VEC, false>), grid, block, dyn, ctx->stream, a); } while (0)
    if (!wide) {
        if (cols <= 256) SN_LAUNCH(1, 1);
        else if (cols <= 512) SN_LAUNCH(1, 2);
        else SN_LAUNCH(1, 4);
    } else {
        if (cols <= 1024) SN_LAUNCH(4, 1);
        else if (cols <= 2048) SN_LAUNCH(4, 2);
        else if (cols <= 4096) SN_LAUNCH(4, 4);
        else SN_LAUNCH(4, 8);
    }
#undef SN_LAUNCH
    RTEN_LAUNCH_CHECK(ctx, "skip_norm_kernel");
    return RTEN_HIP_OK;
}

// ------------------------------------------------------------------------------------------------
// RotaryEmbedding (embedding.rs:144-194)
// ------------------------------------------------------------------------------------------------
struct RotaryArgs {
    int batch, seq, heads, head_size, rotary_dim, interleaved;
    int pos_mode, max_pos; // 0: caches indexed by (b, s) through their strides; 1: position_ids [B, S]; 2: one-element offset k, token s uses k + s
    int64_t x_sb, x_ss, x_sh, y_sb, y_ss, y_sh, cos_sb, cos_ss, sin_sb, sin_ss;
    const float *x, *cos, *sin;
    const int32_t *pos;
    float *y;
    int64_t total; // work items
    int items;     // per row
};

// y1 = x1 * c - x2 * s, y2 = x1 * s + x2 * c with every product and the sum rounded on its own (Rust does not contract)
__device__ __forceinline__ void rot1(float x1, float x2, float c, float s, float &y1, float &y2) {
    y1 = __fsub_rn(__fmul_rn(x1, c), __fmul_rn(x2, s));
    y2 = __fadd_rn(__fmul_rn(x1, s), __fmul_rn(x2, c));
}

template <bool VECF>
__global__ __launch_bounds__(256) void rotary_kernel(const RotaryArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total) return;
    const int64_t row = idx / p.items;
    const int item = (int)(idx - row * p.items);
    const int h = (int)(row % p.heads);
    const int64_t bs = row / p.heads;
    const int s = (int)(bs % p.seq), b = (int)(bs / p.seq);
    const float *xr = p.x + b * p.x_sb + s * p.x_ss + h * p.x_sh;
    float *yr = p.y + b * p.y_sb + s * p.y_ss + h * p.y_sh;
    const int half = p.rotary_dim / 2;
    constexpr int W = VECF ? 4 : 1;
    const int rot_items = half / W;
    if (item >= rot_items) { // the elements from rotary_dim on are copied
        const int i = p.rotary_dim + (item - rot_items) * W;
        if constexpr (VECF) *reinterpret_cast<float4 *>(yr + i) = *reinterpret_cast<const float4 *>(xr + i);
        else yr[i] = xr[i];
        return;
    }
    int64_t co, so;
    if (p.pos_mode == 0) {
        co = b * p.cos_sb + s * p.cos_ss;
        so = b * p.sin_sb + s * p.sin_ss;
    } else {
        // the cache row is gathered here, by the rule of Gather on device data: a negative id counts from the end, then the id is clamped into the axis
        int id = p.pos_mode == 1 ? p.pos[(int64_t)b * p.seq + s] : p.pos[0] + s;
        if (id < 0) id += p.max_pos;
        id = id < 0 ? 0 : (id >= p.max_pos ? p.max_pos - 1 : id);
        co = so = (int64_t)id * half;
    }
    const int i = item * W;
    if constexpr (VECF) {
        const float4 c = *reinterpret_cast<const float4 *>(p.cos + co + i), sn = *reinterpret_cast<const float4 *>(p.sin + so + i);
        if (p.interleaved) {
            const float4 a = *reinterpret_cast<const float4 *>(xr + 2 * i), d = *reinterpret_cast<const float4 *>(xr + 2 * i + 4);
            float4 ya, yd;
            rot1(a.x, a.y, c.x, sn.x, ya.x, ya.y);
            rot1(a.z, a.w, c.y, sn.y, ya.z, ya.w);
            rot1(d.x, d.y, c.z, sn.z, yd.x, yd.y);
            rot1(d.z, d.w, c.w, sn.w, yd.z, yd.w);
            *reinterpret_cast<float4 *>(yr + 2 * i) = ya;
            *reinterpret_cast<float4 *>(yr + 2 * i + 4) = yd;
        } else {
            const float4 a = *reinterpret_cast<const float4 *>(xr + i), d = *reinterpret_cast<const float4 *>(xr + half + i);
            float4 ya, yd;
            rot1(a.x, d.x, c.x, sn.x, ya.x, yd.x);
            rot1(a.y, d.y, c.y, sn.y, ya.y, yd.y);
            rot1(a.z, d.z, c.z, sn.z, ya.z, yd.z);
            rot1(a.w, d.w, c.w, sn.w, ya.w, yd.w);
            *reinterpret_cast<float4 *>(yr + i) = ya;
            *reinterpret_cast<float4 *>(yr + half + i) = yd;
        }
    } else {
        const float c = p.cos[co + i], sn = p.sin[so + i];
        const int i1 = p.interleaved ? 2 * i : i, i2 = p.interleaved ? 2 * i + 1 : half + i;
        float y1, y2;
        rot1(xr[i1], xr[i2], c, sn, y1, y2);
        yr[i1] = y1;
        yr[i2] = y2;
    }
}

} // namespace

RTEN_EXPORT int32_t rten_hip_rms_norm_f32(rten_hip_ctx *ctx, int64_t rows, int32_t cols, const float *x, const float *gamma, float gamma_scalar,
                                          float epsilon, float *y) {
    NormArgs a{};
    a.rows = rows; a.cols = cols; a.x = x; a.gamma = gamma; a.gamma_scalar = gamma ? 1.0f : gamma_scalar; a.eps = epsilon; a.y = y;
    return skip_norm_launch(ctx, "rms_norm_f32", false, a);
}

RTEN_EXPORT int32_t rten_hip_skip_norm_f32(rten_hip_ctx *ctx, int32_t mode, int64_t rows, int32_t cols, const float *x, const float *skip,
                                           int64_t skip_rows, const float *bias, const float *gamma, const float *beta, float epsilon,
                                           float *sum_out, float *y) {
    if (mode != RTEN_HIP_SKIP_NORM_LAYER && mode != RTEN_HIP_SKIP_NORM_RMS) return RTEN_HIP_ERR_INVALID_VALUE;
    if (!skip || !gamma || (beta && mode == RTEN_HIP_SKIP_NORM_RMS)) return RTEN_HIP_ERR_INVALID_VALUE;
    NormArgs a{};
    a.rows = rows; a.skip_rows = skip_rows; a.cols = cols; a.x = x; a.skip = skip; a.bias = bias; a.gamma = gamma; a.beta = beta;
    a.gamma_scalar = 1.0f; a.eps = epsilon; a.sum_out = sum_out; a.y = y;
    if (rows > 0 && cols > 0 && skip_rows > 0 && rows % skip_rows != 0) return RTEN_HIP_ERR_INVALID_VALUE; // skip covers whole batch rows
    const bool ln = mode == RTEN_HIP_SKIP_NORM_LAYER;
    return skip_norm_launch(ctx, ln ? "skip_layer_norm_f32" : "skip_rms_norm_f32", ln, a);
}

RTEN_EXPORT int32_t rten_hip_rotary_embedding_f32(rten_hip_ctx *ctx, int32_t batch, int32_t seq, int32_t heads, int32_t head_size, int32_t rotary_dim,
                                                  int32_t interleaved, const float *x, int64_t x_stride_b, int64_t x_stride_s, int64_t x_stride_h,
                                                  const float *cos, int64_t cos_stride_b, int64_t cos_stride_s, const float *sin, int64_t sin_stride_b,
                                                  int64_t sin_stride_s, const int32_t *position_ids, int32_t position_mode, int32_t max_pos, float *y,
                                                  int64_t y_stride_b, int64_t y_stride_s, int64_t y_stride_h) {
    RTEN_CHECK_CTX(ctx);
    if (batch < 0 || seq < 0 || heads < 0 || head_size < 0) return RTEN_HIP_ERR_INVALID_VALUE;
    if (rotary_dim < 0 || rotary_dim % 2 != 0 || rotary_dim > head_size) return RTEN_HIP_ERR_INVALID_VALUE;
    if (position_mode < RTEN_HIP_ROTARY_POS_NONE || position_mode > RTEN_HIP_ROTARY_POS_OFFSET) return RTEN_HIP_ERR_INVALID_VALUE;
    const int64_t rows = (int64_t)batch * seq * heads;
    if (rows == 0 || head_size == 0) return RTEN_HIP_OK;
    if (!x || !y) return RTEN_HIP_ERR_INVALID_VALUE;
    if (rotary_dim > 0 && (!cos || !sin)) return RTEN_HIP_ERR_INVALID_VALUE;
    if (position_mode != RTEN_HIP_ROTARY_POS_NONE && rotary_dim > 0 && (!position_ids || max_pos <= 0)) return RTEN_HIP_ERR_INVALID_VALUE;
    const int half = rotary_dim / 2;
    auto mult4 = [](int64_t v) { return v % 4 == 0; };
    const bool cache_ok = position_mode != RTEN_HIP_ROTARY_POS_NONE || (mult4(cos_stride_b) && mult4(cos_stride_s) && mult4(sin_stride_b) && mult4(sin_stride_s));
    const bool vec = half % 4 == 0 && head_size % 4 == 0 && mult4(x_stride_b) && mult4(x_stride_s) && mult4(x_stride_h) && mult4(y_stride_b) &&
                     mult4(y_stride_s) && mult4(y_stride_h) && cache_ok && aligned16(x) && aligned16(y) && aligned16(cos) && aligned16(sin);
    RotaryArgs a{};
    a.batch = batch; a.seq = seq; a.heads = heads; a.head_size = head_size; a.rotary_dim = rotary_dim; a.interleaved = interleaved != 0;
    a.pos_mode = position_mode; a.max_pos = max_pos;
    a.x_sb = x_stride_b; a.x_ss = x_stride_s; a.x_sh = x_stride_h; a.y_sb = y_stride_b; a.y_ss = y_stride_s; a.y_sh = y_stride_h;
    a.cos_sb = cos_stride_b; a.cos_ss = cos_stride_s; a.sin_sb = sin_stride_b; a.sin_ss = sin_stride_s;
    a.x = x; a.cos = cos; a.sin = sin; a.pos = position_ids; a.y = y;
    a.items = vec ? half / 4 + (head_size - rotary_dim) / 4 : half + (head_size - rotary_dim);
    a.total = rows * a.items;
    ProfScope ps(ctx, "rotary_embedding_f32", 6.0 * rows * half, 8.0 * rows * head_size);
    const dim3 grid((unsigned)ceil_div64(a.total, 256)), block(256);
    if (vec) hipLaunchKernelGGL(rotary_kernel<true>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(rotary_kernel<false>, grid, block, 0, ctx->stream, a);
    RTEN_LAUNCH_CHECK(ctx, "rotary_kernel");
    return RTEN_HIP_OK;
}
