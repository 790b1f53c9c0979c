// InstanceNormalization, LogSoftmax and the activation form of BatchNormalization.
// Replaces src/ops/norm.rs:103-161,164-189,320-365 (instance normalisation = normalize_each over N*C slices),
// rten-vecmath/src/normalize.rs:112-127, rten-vecmath/src/softmax.rs:131-174 and norm.rs:194-224.
//
// InstanceNormalization has few, long slices (N*C rows of H*W elements).  Per slice r = b*C + ch:
//   mean = Sum(row) / inner ; var = SumSquareSub(row, mean) / inner ; s = scale[ch] / sqrtf(var + eps) ;
//   y = act(fma(x - mean, s, bias[ch]))
// Each of the 64 accumulator slots (u, l) of the two reductions is a strictly sequential chain over the elements
// i = 16u + l (mod 64) (rowreduce.h), so the reductions of one slice belong to ONE wavefront; loading the slice and the
// normalise pass are free to use the whole workgroup.  Three forms:
//   register  inner <= 1024: one wave per slice, the slice in registers (layer_norm_kernel's shape), four slices per workgroup
//   resident  inner <= RTEN_HIP_INSTANCE_NORM_RESIDENT_MAX: one workgroup per slice; all waves bring it into LDS, wave 0 reduces
//             from LDS, all waves normalise LDS -> y: one read and one write per element
//   streaming any inner: wave 0 reduces from memory with many loads in flight per lane, all waves normalise memory -> y
// No workgroup waits for another, no atomics, no scratch: every form can be captured.  y may equal x (slices are disjoint and a
// workgroup stores only behind the barrier that ends its reductions; the normalise pass reads each element before its own store).
#include <cmath>

#include "internal.h"
#include "rowreduce.h"
#include "vecmath.h"

namespace {

constexpr int ROWS_PER_BLOCK = 4;
constexpr int IN_THREADS = 512;  // resident / streaming workgroup: 8 waves, so 2 (LDS > 40 KiB) to 4 workgroups share a compute unit
constexpr int STREAM_BATCH = 32; // loads in flight per lane of the reducing wave (8 KiB per wave)
constexpr int LDS_BATCH = 8;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// register form
// ------------------------------------------------------------------------------------------------
template <int CH>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void instance_norm_reg_kernel(int64_t rows, int c, int cols, const float *x, const float *__restrict__ scale,
                                                                                const float *__restrict__ bias, float eps, int act, float aa, float ab, float *y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *xr = x + row * cols;
    float *yr = y + row * cols;
    const int ch = (int)(row % c);
    const float sc = scale[ch], bi = bias[ch]; // requested with the row: they depend on nothing
    float v[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) { const int i = k * 64 + lane; v[k] = i < cols ? xr[i] : 0.f; }
    auto get = [&](int i) -> float { return xr[i]; }; // the < 64-element remainder: cross-lane, served from L1 (read before any store of this wave)
    auto red = [&](auto f) -> float {
        float acc = 0.f;
        const int full4 = cols / 64;
#pragma unroll
        for (int k = 0; k < CH; k++)
            if (k < full4) acc = f(acc, v[k]);
        float a = acc;
        a = a + lane_bcast(acc, (lane & 15) + 16);
        a = a + lane_bcast(acc, (lane & 15) + 32);
        a = a + lane_bcast(acc, (lane & 15) + 48);
        int i0 = full4 * 64;
        const int l = lane & 15;
        for (; i0 + 16 <= cols; i0 += 16) a = f(a, get(i0 + l));
        if (i0 + l < cols) a = f(a, get(i0 + l));
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; k++) s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), k));
        return s;
    };
    const float mean = red([](float acc, float xv) { return acc + xv; }) / (float)cols;
    const float var = red([mean](float acc, float xv) { const float d = xv - mean; return vm::fma(d, d, acc); }) / (float)cols;
    const float ssr = sc / sqrtf(var + eps);
#pragma unroll
    for (int k = 0; k < CH; k++) v[k] = vm::fma(v[k] - mean, ssr, bi);
    vm::activation_n<CH>(act, v, aa, ab);
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const int i = k * 64 + lane;
        if (i < cols) yr[i] = v[k];
    }
}

// The normalise pass of the two workgroup forms: src (LDS or memory) -> y, 16 bytes per lane where the slice allows.
template <typename Src>
__device__ __forceinline__ void normalise_pass(Src src, bool vec4, int64_t inner, float mean, float ssr, float bi, int act, float aa, float ab, float *yr) {
    if (vec4) {
        const int64_t n4 = inner >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += IN_THREADS) {
            f32x4 t = reinterpret_cast<const f32x4 *>(src)[i];
#pragma unroll
            for (int k = 0; k < 4; k++) t[k] = vm::fma(t[k] - mean, ssr, bi);
            vm::activation_n<4>(act, t, aa, ab);
            reinterpret_cast<f32x4 *>(yr)[i] = t;
        }
    } else {
        for (int64_t i = threadIdx.x; i < inner; i += IN_THREADS) yr[i] = vm::activation(act, vm::fma(src[i] - mean, ssr, bi), aa, ab);
    }
}

// ------------------------------------------------------------------------------------------------
// resident form: dynamic LDS = the slice (inner floats, rounded up to 16 bytes)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IN_THREADS) void instance_norm_resident_kernel(int c, int inner, const float *x, const float *__restrict__ scale,
                                                                            const float *__restrict__ bias, float eps, int act, float aa, float ab, float *y,
                                                                            int vec4) {
    extern __shared__ f32x4 in_slice4[];
    __shared__ float stat[2];
    float *s = reinterpret_cast<float *>(in_slice4);
    const int64_t row = blockIdx.x;
    const float *xr = x + row * inner;
    const int ch = (int)(row % c);
    const float sc = scale[ch], bi = bias[ch];
    if (vec4) {
        const int n4 = inner >> 2;
        for (int i = threadIdx.x; i < n4; i += IN_THREADS) in_slice4[i] = reinterpret_cast<const f32x4 *>(xr)[i];
    } else {
        for (int i = threadIdx.x; i < inner; i += IN_THREADS) s[i] = xr[i];
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        auto get = [&](int i) -> float { return s[i]; };
        const float mean = simd16_reduce<0, LDS_BATCH>(get, inner, 0.f, lane) / (float)inner;
        const float var = simd16_reduce<1, LDS_BATCH>(get, inner, mean, lane) / (float)inner;
        if (lane == 0) { stat[0] = mean; stat[1] = sc / sqrtf(var + eps); }
    }
    __syncthreads();
    normalise_pass(s, vec4 != 0, inner, stat[0], stat[1], bi, act, aa, ab, y + row * inner);
}

// ------------------------------------------------------------------------------------------------
// streaming form
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IN_THREADS) void instance_norm_stream_kernel(int c, int64_t inner, const float *x, const float *__restrict__ scale,
                                                                          const float *__restrict__ bias, float eps, int act, float aa, float ab, float *y, int vec4) {
    __shared__ float stat[2];
    const int64_t row = blockIdx.x;
    const float *xr = x + row * inner;
    const int ch = (int)(row % c);
    const float sc = scale[ch], bi = bias[ch];
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        auto get = [&](int64_t i) -> float { return xr[i]; };
        const float mean = simd16_reduce<0, STREAM_BATCH>(get, inner, 0.f, lane) / (float)inner;
        const float var = simd16_reduce<1, STREAM_BATCH>(get, inner, mean, lane) / (float)inner;
        if (lane == 0) { stat[0] = mean; stat[1] = sc / sqrtf(var + eps); }
    }
    __syncthreads(); // no store of this workgroup before its reductions have read the slice (y may be x)
    normalise_pass(xr, vec4 != 0, inner, stat[0], stat[1], bi, act, aa, ab, y + row * inner);
}

// y = act(fma(x - mean_c, scale_c / sqrt(var_c + eps), bias_c))  (norm.rs:194-224 + normalize.rs:112-127, then the activation on the same f32 value)
__global__ __launch_bounds__(256) void batch_norm_act_kernel(int64_t total, int c, int64_t inner, const float *__restrict__ x, const float *__restrict__ scale,
                                                             const float *__restrict__ bias, const float *__restrict__ mean, const float *__restrict__ var,
                                                             float eps, int act, float aa, float ab, float *__restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int ch = (int)((i / inner) % c);
        const float ssr = scale[ch] / sqrtf(var[ch] + eps);
        y[i] = vm::activation(act, vm::fma(x[i] - mean[ch], ssr, bias[ch]), aa, ab);
    }
}

// ------------------------------------------------------------------------------------------------
// LogSoftmax (softmax.rs:131-174): max (f32::MIN start), sum of ReducedRangeExp(x - max) in the single-accumulator 16-lane order of
// the softmax kernels (rowwise.hip), y = (x - max) - ln(sum): two subtractions.  ln: the f64 logarithm of the sum rounded to f32, once per row
// (the reference calls the host's libm logf; docs/KERNELS.md 4.7).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ordered_lane_total(float a) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k++) s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), k));
    return s;
}

template <int CH>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void log_softmax_kernel(int64_t rows, int cols, const float *x, float *y) {
    const int lane = threadIdx.x & 63, l = lane & 15;
    const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *xr = x + row * cols;
    float *yr = y + row * cols;
    float v[CH];
    float mx = -3.40282347e+38f; // f32::MIN (softmax.rs:136)
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const int i = k * 64 + lane;
        float t = -3.40282347e+38f;
        if (i < cols) { t = xr[i]; mx = fmaxf(mx, t); }
        v[k] = t;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const int i = k * 64 + lane;
        v[k] = v[k] - mx;
        const float e = i < cols ? vm::exp_reduced(v[k]) : 0.f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float eq = lane_bcast(e, l + 16 * q);
            if (k * 64 + l + 16 * q < cols) a = a + eq;
        }
    }
    const float lg = (float)log((double)ordered_lane_total(a));
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const int i = k * 64 + lane;
        if (i < cols) yr[i] = v[k] - lg;
    }
}

// Long rows: the same order, the row re-read (L2 resident).  y may equal x: a wave stores only after its last read of the row.
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void log_softmax_long_kernel(int64_t rows, int cols, const float *x, float *y) {
    const int lane = threadIdx.x & 63, l = lane & 15;
    const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *xr = x + row * cols;
    float *yr = y + row * cols;
    float mx = -3.40282347e+38f;
    for (int i = lane; i < cols; i += 64) mx = fmaxf(mx, xr[i]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float a = 0.f;
    const int nch = (cols + 63) / 64;
    for (int k = 0; k < nch; k++) {
        const int i = k * 64 + lane;
        const float e = i < cols ? vm::exp_reduced(xr[i] - mx) : 0.f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float eq = lane_bcast(e, l + 16 * q);
            if (k * 64 + l + 16 * q < cols) a = a + eq;
        }
    }
    const float lg = (float)log((double)ordered_lane_total(a));
    for (int i = lane; i < cols; i += 64) yr[i] = (xr[i] - mx) - lg;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

} // namespace

RTEN_EXPORT int32_t rten_hip_set_instance_norm_path(rten_hip_ctx *ctx, int32_t mode) {
    RTEN_CHECK_CTX(ctx);
    if (mode < 0 || mode > 2) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "set_instance_norm_path: mode must be 0, 1 or 2");
    ctx->instance_norm_path = mode;
    return RTEN_HIP_OK;
}

RTEN_EXPORT int32_t rten_hip_instance_norm_f32(rten_hip_ctx *ctx, int32_t n, int32_t c, int64_t inner, const float *x, const float *scale, const float *bias,
                                               float epsilon, int32_t act_kind, float act_alpha, float act_beta, float *y) {
    RTEN_CHECK_CTX(ctx);
    if (n < 0 || c < 0 || inner < 0) return RTEN_HIP_ERR_INVALID_VALUE;
    if (!rten_act_valid(act_kind)) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "instance_norm: unknown activation kind %d", act_kind);
    const int64_t rows = (int64_t)n * c;
    if (rows == 0 || inner == 0) return RTEN_HIP_OK;
    if (!x || !scale || !bias || !y) return RTEN_HIP_ERR_INVALID_VALUE;
    if (rows > 0x7fffffff) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "instance_norm: more than 2^31 - 1 slices");
    ProfScope ps(ctx, "instance_norm_f32", 0.0, 8.0 * rows * inner);
    const int mode = ctx->instance_norm_path;
    // automatic: the register form for short slices, the streaming form above them.  The resident form has not been timed against the streaming
    // form yet (docs/KERNELS.md 4.7), so it is opt-in (mode 2); where a slice does not fit it, mode 2 streams.
    const bool resident = mode == 2 && inner <= RTEN_HIP_INSTANCE_NORM_RESIDENT_MAX;
    const int vec4 = (inner % 4 == 0 && aligned16(x) && aligned16(y)) ? 1 : 0;
    if (mode == 0 && inner <= 1024) {
        const dim3 grid((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), block(64 * ROWS_PER_BLOCK);
        const int cols = (int)inner;
#define IN_LAUNCH(CH) hipLaunchKernelGGL((instance_norm_reg_kernel<CH>), grid, block, 0, ctx->stream, rows, c, cols, x, scale, bias, epsilon, act_kind, act_alpha, act_beta, y)
        if (cols <= 64) IN_LAUNCH(1);
        else if (cols <= 128) IN_LAUNCH(2);
        else if (cols <= 256) IN_LAUNCH(4);
        else if (cols <= 512) IN_LAUNCH(8);
        else IN_LAUNCH(16);
#undef IN_LAUNCH
        RTEN_LAUNCH_CHECK(ctx, "instance_norm_reg_kernel");
    } else if (resident) {
        const size_t lds = (((size_t)inner + 3) / 4) * 16;
        if (lds > 64 * 1024) // (per function and device; as layer_norm_launch does)
            RTEN_HIP_TRY(ctx, hipFuncSetAttribute((const void *)instance_norm_resident_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTEN_HIP_INSTANCE_NORM_RESIDENT_MAX * 4));
        hipLaunchKernelGGL(instance_norm_resident_kernel, dim3((unsigned)rows), dim3(IN_THREADS), lds, ctx->stream, c, (int)inner, x, scale, bias, epsilon, act_kind,
                           act_alpha, act_beta, y, vec4);
        RTEN_LAUNCH_CHECK(ctx, "instance_norm_resident_kernel");
    } else {
        hipLaunchKernelGGL(instance_norm_stream_kernel, dim3((unsigned)rows), dim3(IN_THREADS), 0, ctx->stream, c, inner, x, scale, bias, epsilon, act_kind, act_alpha,
                           act_beta, y, vec4);
        RTEN_LAUNCH_CHECK(ctx, "instance_norm_stream_kernel");
    }
    return RTEN_HIP_OK;
}

RTEN_EXPORT int32_t rten_hip_batch_norm_f32_act(rten_hip_ctx *ctx, int32_t n, int32_t c, int64_t inner, const float *x, const float *scale, const float *bias,
                                                const float *mean, const float *var, float epsilon, int32_t act_kind, float act_alpha, float act_beta, float *y) {
    RTEN_CHECK_CTX(ctx);
    if (!rten_act_valid(act_kind)) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "batch_norm: unknown activation kind %d", act_kind);
    if (n < 0 || c <= 0 || inner < 0) return RTEN_HIP_ERR_INVALID_VALUE;
    const int64_t total = (int64_t)n * c * inner;
    if (total == 0) return RTEN_HIP_OK;
    if (!x || !scale || !bias || !mean || !var || !y) return RTEN_HIP_ERR_INVALID_VALUE;
    ProfScope ps(ctx, act_kind == RTEN_HIP_ACT_NONE ? "batch_norm_f32" : "batch_norm_f32_act", 0.0, 8.0 * total);
    const int64_t blocks = (total + 255) / 256; // (grid-stride loop, at most 2048 workgroups: the element-wise kernels' launch shape)
    hipLaunchKernelGGL(batch_norm_act_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, ctx->stream, total, c, inner, x, scale, bias, mean, var,
                       epsilon, act_kind, act_alpha, act_beta, y);
    RTEN_LAUNCH_CHECK(ctx, "batch_norm_act_kernel");
    return RTEN_HIP_OK;
}

RTEN_EXPORT int32_t rten_hip_log_softmax_f32(rten_hip_ctx *ctx, int64_t rows, int32_t cols, const float *x, float *y) {
    RTEN_CHECK_CTX(ctx);
    if (rows < 0 || cols < 0) return RTEN_HIP_ERR_INVALID_VALUE;
    if (rows == 0 || cols == 0) return RTEN_HIP_OK;
    if (!x || !y) return RTEN_HIP_ERR_INVALID_VALUE;
    const int64_t blocks = (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    if (blocks > 0x7fffffff) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "log_softmax: more than 2^33 rows");
    const dim3 grid((unsigned)blocks), block(64 * ROWS_PER_BLOCK);
    ProfScope ps(ctx, "log_softmax_f32", 0.0, 8.0 * rows * cols);
#define LSM_LAUNCH(CH) hipLaunchKernelGGL((log_softmax_kernel<CH>), grid, block, 0, ctx->stream, rows, cols, x, y)
    if (cols <= 64) LSM_LAUNCH(1);
    else if (cols <= 128) LSM_LAUNCH(2);
    else if (cols <= 256) LSM_LAUNCH(4);
    else if (cols <= 512) LSM_LAUNCH(8);
    else if (cols <= 1024) LSM_LAUNCH(16);
    else hipLaunchKernelGGL(log_softmax_long_kernel, grid, block, 0, ctx->stream, rows, cols, x, y);
#undef LSM_LAUNCH
    RTEN_LAUNCH_CHECK(ctx, "log_softmax_kernel");
    return RTEN_HIP_OK;
}
