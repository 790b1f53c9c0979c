// QuantizeLinear, DequantizeLinear and their round trip (HBM-bound).  Replaces src/ops/quantize.rs:19-334 and, for u8, rten-vecmath/src/quantize.rs.
//
// Geometry: [outer][channels][inner], element (o, c, i) uses scale[c] / zero_point[c] (device pointers: nothing is read back); channels == 1 is per-tensor.
// Two kernels, neither with an integer division per element:
//   qdq_plane_kernel   blockIdx.y walks the outer * channels planes (one `%` per plane for c; none when channels == 1, where the one plane is the whole
//                      tensor), blockIdx.x and the lanes walk `inner` as a grid-stride loop of 4-element vectors -- 16 B of f32 / int32, 4 B of u8 / i8 per
//                      lane per access -- between a scalar head and tail.  The head is chosen per plane from both operands' addresses (operands are views at
//                      any element offset into a pooled buffer, the 8-bit one at any byte; planes of an odd `inner` start at every alignment); where no head
//                      of 0-3 elements aligns both, that plane moves element by element.
//   qdq_lastaxis_kernel  inner == 1 (quantisation along the last axis): a lane owns 4 adjacent channels (1 where channels % 4 != 0 or an operand is
//                      misaligned), keeps their scale / 1 / scale / zero point in registers and walks the rows.
// Grid capped at 2048 x-blocks (256 CUs x 8), y so that the product stays near it.
//
// Arithmetic (-ffp-contract=off, hipcc's correctly rounded f32 division): inv_scale = 1.0f / scale[c]; quantize = saturate(rint(x * inv_scale) + zp);
// dequantize = (float)(int32 wrapping x - zp) * scale[c].  u8 goes through dql::quant_u8 (quantize.h), the statement of rten-vecmath's u8 kernel; for i8, and
// for what the scalar definition (quantize.rs:171-194) does differently outside |x * inv_scale| < 2^31, see quant_one.  docs/KERNELS.md 4.9.
#include <algorithm>
#include <type_traits>

#include "internal.h"
#include "quantize.h"

typedef int qdq_i32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int QDQ_THREADS = 256;
constexpr int QDQ_GRID_CAP = 2048;
enum { QDQ_QUANTIZE = 0, QDQ_DEQUANTIZE = 1, QDQ_ROUND_TRIP = 2 };

template <int DT> struct QType;
template <> struct QType<RTEN_HIP_DT_U8> { using T = uint8_t; };
template <> struct QType<RTEN_HIP_DT_I8> { using T = int8_t; };
template <> struct QType<RTEN_HIP_DT_I32> { using T = int32_t; };

// PT (channels == 1) u8: rten-vecmath's kernel, i.e. quant_u8 for every input.  Per-axis u8 is the reference's scalar loop, which differs from it in one
// place: a product >= 2^31 (+inf included) saturates to 255.  i8 is the scalar definition taken literally: the zero point is added in f32, then a saturating
// cast (NaN -> 0).
template <int DT, bool PT>
__device__ __forceinline__ int quant_one(float x, float inv_scale, int zp) {
    if constexpr (DT == RTEN_HIP_DT_U8) {
        const unsigned q = dql::quant_u8(x, inv_scale, zp);
        if constexpr (PT) return (int)q;
        else return x * inv_scale >= 2147483648.f ? 255 : (int)q;
    } else {
        const float r = rintf(x * inv_scale) + (float)zp;
        const float c = fminf(fmaxf(r, -128.f), 127.f);
        return r != r ? 0 : (int)c;
    }
}
__device__ __forceinline__ float dequant_one(int q, int zp, float scale) { return (float)(int)((unsigned)q - (unsigned)zp) * scale; }

template <int KIND, int DT, bool PT>
struct QdqOp {
    using Q = typename QType<DT>::T;
    using In = typename std::conditional<KIND == QDQ_DEQUANTIZE, Q, float>::type;
    using Out = typename std::conditional<KIND == QDQ_QUANTIZE, Q, float>::type;
    float scale, inv_scale;
    int zp;
    __device__ __forceinline__ void load(const float *s, const void *z, int64_t c) {
        scale = s[c];
        zp = z ? (int)static_cast<const Q *>(z)[c] : 0;
        inv_scale = KIND == QDQ_DEQUANTIZE ? 0.f : 1.0f / scale; // quantize.rs:210,262
    }
    __device__ __forceinline__ Out operator()(In v) const {
        if constexpr (KIND == QDQ_DEQUANTIZE) return dequant_one((int)v, zp, scale);
        else if constexpr (KIND == QDQ_QUANTIZE) return (Out)quant_one<DT, PT>(v, inv_scale, zp);
        else return dequant_one((int)(Q)quant_one<DT, PT>(v, inv_scale, zp), zp, scale);
    }
};

// 4 consecutive elements: one 16-byte access of a 4-byte type, one 4-byte access of an 8-bit type.  `p` is aligned to the access.
template <typename T>
__device__ __forceinline__ void load4(const T *p, T (&v)[4]) {
    if constexpr (sizeof(T) == 4) {
        const qdq_i32x4 w = *reinterpret_cast<const qdq_i32x4 *>(p);
#pragma unroll
        for (int k = 0; k < 4; k++) { const int e = w[k]; __builtin_memcpy(&v[k], &e, 4); }
    } else {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (T)((w >> (8 * k)) & 0xffu);
    }
}
template <typename T>
__device__ __forceinline__ void store4(T *p, const T (&v)[4]) {
    if constexpr (sizeof(T) == 4) {
        qdq_i32x4 w;
#pragma unroll
        for (int k = 0; k < 4; k++) { int e; __builtin_memcpy(&e, &v[k], 4); w[k] = e; }
        *reinterpret_cast<qdq_i32x4 *>(p) = w;
    } else {
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) w |= (uint32_t)(uint8_t)v[k] << (8 * k);
        *reinterpret_cast<uint32_t *>(p) = w;
    }
}
template <typename A, typename B>
__device__ __host__ __forceinline__ bool aligned4(const A *a, const B *b) {
    return ((uintptr_t)a & (4 * sizeof(A) - 1)) == 0 && ((uintptr_t)b & (4 * sizeof(B) - 1)) == 0;
}

// No __restrict__: y may equal x in the round trip (every element is read before it is written, by the same lane).
template <int KIND, int DT, bool PT>
__global__ __launch_bounds__(QDQ_THREADS) void qdq_plane_kernel(int64_t planes, int64_t channels, int64_t inner, const void *xv, const float *scale, const void *zpv,
                                                                void *yv) {
    using Op = QdqOp<KIND, DT, PT>;
    using In = typename Op::In;
    using Out = typename Op::Out;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t p = blockIdx.y; p < planes; p += gridDim.y) {
        Op op;
        op.load(scale, zpv, PT ? 0 : p % channels);
        const In *x = static_cast<const In *>(xv) + p * inner;
        Out *y = static_cast<Out *>(yv) + p * inner;
        int head = -1; // scalar elements before the first vector both operands can take, or -1: none
#pragma unroll
        for (int h = 3; h >= 0; h--)
            if (aligned4(x + h, y + h)) head = h;
        if (inner - head < 4) head = -1;
        if (head < 0) {
            for (int64_t i = tid; i < inner; i += stride) y[i] = op(x[i]);
            continue;
        }
        const int64_t n4 = (inner - head) >> 2;
        for (int64_t i = tid; i < n4; i += stride) {
            In v[4];
            Out r[4];
            load4(x + head + 4 * i, v);
#pragma unroll
            for (int k = 0; k < 4; k++) r[k] = op(v[k]);
            store4(y + head + 4 * i, r);
        }
        if (tid < head) y[tid] = op(x[tid]);
        for (int64_t i = head + (n4 << 2) + tid; i < inner; i += stride) y[i] = op(x[i]);
    }
}

// inner == 1, channels > 1.  VEC: channels % 4 == 0 and both bases aligned to a 4-element access, so every row's vectors are.
template <int KIND, int DT, bool VEC>
__global__ __launch_bounds__(QDQ_THREADS) void qdq_lastaxis_kernel(int64_t rows, int64_t channels, const void *xv, const float *scale, const void *zpv, void *yv) {
    using Op = QdqOp<KIND, DT, false>;
    using In = typename Op::In;
    using Out = typename Op::Out;
    constexpr int W = VEC ? 4 : 1;
    const In *x = static_cast<const In *>(xv);
    Out *y = static_cast<Out *>(yv);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * W;
    for (int64_t c = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * W; c < channels; c += stride) {
        Op op[W];
#pragma unroll
        for (int k = 0; k < W; k++) op[k].load(scale, zpv, c + k);
        for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
            const int64_t at = r * channels + c;
            if constexpr (VEC) {
                In v[4];
                Out o[4];
                load4(x + at, v);
#pragma unroll
                for (int k = 0; k < 4; k++) o[k] = op[k](v[k]);
                store4(y + at, o);
            } else {
                y[at] = op[0](x[at]);
            }
        }
    }
}

inline int ceil_cap(int64_t items, int64_t per, int64_t cap) {
    int64_t b = (items + per - 1) / per;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

template <int KIND, int DT>
void qdq_launch(rten_hip_ctx *ctx, int64_t outer, int64_t channels, int64_t inner, const void *x, const float *scale, const void *zp, void *y) {
    using In = typename QdqOp<KIND, DT, false>::In;
    using Out = typename QdqOp<KIND, DT, false>::Out;
    const dim3 block(QDQ_THREADS);
    if (channels > 1 && inner == 1) {
        const bool vec = channels % 4 == 0 && aligned4(static_cast<const In *>(x), static_cast<Out *>(y));
        const int gx = ceil_cap(channels, (vec ? 4 : 1) * QDQ_THREADS, QDQ_GRID_CAP);
        const int gy = ceil_cap(outer, 8, std::max(1, QDQ_GRID_CAP / gx)); // 8 rows or more per lane: the division for 1 / scale is paid once per lane
        if (vec) hipLaunchKernelGGL((qdq_lastaxis_kernel<KIND, DT, true>), dim3(gx, gy), block, 0, ctx->stream, outer, channels, x, scale, zp, y);
        else hipLaunchKernelGGL((qdq_lastaxis_kernel<KIND, DT, false>), dim3(gx, gy), block, 0, ctx->stream, outer, channels, x, scale, zp, y);
        return;
    }
    if (channels == 1) { // per-tensor: one plane
        const int gx = ceil_cap(outer * inner, 4 * QDQ_THREADS, QDQ_GRID_CAP);
        hipLaunchKernelGGL((qdq_plane_kernel<KIND, DT, true>), dim3(gx, 1), block, 0, ctx->stream, (int64_t)1, (int64_t)1, outer * inner, x, scale, zp, y);
        return;
    }
    const int gx = ceil_cap(inner, 4 * QDQ_THREADS, QDQ_GRID_CAP);
    const int gy = ceil_cap(outer * channels, 1, std::max(1, 2 * QDQ_GRID_CAP / gx));
    hipLaunchKernelGGL((qdq_plane_kernel<KIND, DT, false>), dim3(gx, gy), block, 0, ctx->stream, outer * channels, channels, inner, x, scale, zp, y);
}

template <int KIND>
int32_t qdq_entry(rten_hip_ctx *ctx, const char *what, int32_t dtype, int64_t outer, int64_t channels, int64_t inner, const void *x, const float *scale, const void *zp,
                  void *y) {
    RTEN_CHECK_CTX(ctx);
    const bool dt_ok = dtype == RTEN_HIP_DT_U8 || dtype == RTEN_HIP_DT_I8 || (KIND == QDQ_DEQUANTIZE && dtype == RTEN_HIP_DT_I32);
    if (!dt_ok) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, KIND == QDQ_DEQUANTIZE ? "dequantize_linear: dtype must be u8, i8 or i32" : "quantize_linear: dtype must be u8 or i8");
    if (outer < 0 || channels < 1 || inner < 0) return RTEN_HIP_ERR_INVALID_VALUE;
    if (outer == 0 || inner == 0) return RTEN_HIP_OK;
    if (!x || !y || !scale) return RTEN_HIP_ERR_INVALID_VALUE;
    const bool x32 = KIND != QDQ_DEQUANTIZE || dtype == RTEN_HIP_DT_I32, zp32 = dtype == RTEN_HIP_DT_I32;
    if (((uintptr_t)scale & 3u) || (x32 && ((uintptr_t)x & 3u)) || (KIND != QDQ_QUANTIZE && ((uintptr_t)y & 3u)) || (zp32 && ((uintptr_t)zp & 3u)))
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "quantize / dequantize: a 4-byte operand is not 4-byte aligned");
    const int64_t n = outer * channels * inner;
    const double bytes = (KIND == QDQ_QUANTIZE ? 5.0 : KIND == QDQ_ROUND_TRIP || dtype == RTEN_HIP_DT_I32 ? 8.0 : 5.0) * (double)n;
    ProfScope ps(ctx, what, 0.0, bytes);
    if (dtype == RTEN_HIP_DT_U8) qdq_launch<KIND, RTEN_HIP_DT_U8>(ctx, outer, channels, inner, x, scale, zp, y);
    else if (dtype == RTEN_HIP_DT_I8) qdq_launch<KIND, RTEN_HIP_DT_I8>(ctx, outer, channels, inner, x, scale, zp, y);
    else if constexpr (KIND == QDQ_DEQUANTIZE) qdq_launch<KIND, RTEN_HIP_DT_I32>(ctx, outer, channels, inner, x, scale, zp, y);
    RTEN_LAUNCH_CHECK(ctx, what);
    return RTEN_HIP_OK;
}

} // namespace

RTEN_EXPORT int32_t rten_hip_quantize_linear_f32(rten_hip_ctx *ctx, int32_t dtype, int64_t outer, int64_t channels, int64_t inner, const float *x, const float *scale,
                                                 const void *zero_point, void *y) {
    return qdq_entry<QDQ_QUANTIZE>(ctx, "quantize_linear_f32", dtype, outer, channels, inner, x, scale, zero_point, y);
}

RTEN_EXPORT int32_t rten_hip_dequantize_linear_f32(rten_hip_ctx *ctx, int32_t dtype, int64_t outer, int64_t channels, int64_t inner, const void *x, const float *scale,
                                                   const void *zero_point, float *y) {
    return qdq_entry<QDQ_DEQUANTIZE>(ctx, "dequantize_linear_f32", dtype, outer, channels, inner, x, scale, zero_point, y);
}

RTEN_EXPORT int32_t rten_hip_quantize_dequantize_f32(rten_hip_ctx *ctx, int32_t dtype, int64_t outer, int64_t channels, int64_t inner, const float *x, const float *scale,
                                                     const void *zero_point, float *y) {
    return qdq_entry<QDQ_ROUND_TRIP>(ctx, "quantize_dequantize_f32", dtype, outer, channels, inner, x, scale, zero_point, y);
}
