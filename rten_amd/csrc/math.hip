// Unary math operators (HBM-bound): Neg, Abs, Sign, Floor, Ceil, Round, Sqrt, Reciprocal, Exp, Log, Softplus.  Replaces
// src/ops/unary_elementwise.rs (the unary_float_op! / unary_numeric_op! operators of that file) and rten-vecmath's Exp.
//
// Layout: one kernel instantiation per operator code, so the float64 routines of Log / Softplus (and their registers) stay out of the one-instruction
// operators.  Flat grid-stride loop, 16 B per lane per access between a scalar head and tail when x and y are misaligned by the same amount (operands
// are often views at an element offset into a pooled buffer), 4 B per lane otherwise; grid capped at 256 CUs x 8 workgroups.
//
// Exactness: the library is built with -ffp-contract=off and hipcc's default correctly rounded f32 division and square root, with f32 subnormals kept,
// so Sqrt and Reciprocal are IEEE results (tests/test_gpu_math_pad.py checks subnormal inputs and results).  Log and Softplus are the float64 function
// rounded once to f32 (docs/KERNELS.md 4.8): the reference calls the host's libm there, which is not correctly rounded.
#include "internal.h"
#include "vecmath.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int MATH_THREADS = 256;

inline int math_blocks(int64_t work_items) {
    int64_t b = (work_items + MATH_THREADS - 1) / MATH_THREADS;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

template <int OP>
__device__ __forceinline__ float unary_math(float x) {
    if constexpr (OP == RTEN_HIP_UNARY_NEG) return __int_as_float(__float_as_int(x) ^ (int)0x80000000); // Rust `-x`: the sign bit, NaN included
    else if constexpr (OP == RTEN_HIP_UNARY_ABS) return __int_as_float(__float_as_int(x) & 0x7fffffff);
    else if constexpr (OP == RTEN_HIP_UNARY_SIGN) return x != x ? __builtin_nanf("") : __builtin_copysignf(1.0f, x); // f32::signum
    else if constexpr (OP == RTEN_HIP_UNARY_FLOOR) return __builtin_floorf(x);
    else if constexpr (OP == RTEN_HIP_UNARY_CEIL) return __builtin_ceilf(x);
    else if constexpr (OP == RTEN_HIP_UNARY_ROUND) return __builtin_rintf(x); // round_ties_even (v_rndne_f32)
    else if constexpr (OP == RTEN_HIP_UNARY_SQRT) return __builtin_sqrtf(x);
    else if constexpr (OP == RTEN_HIP_UNARY_RECIPROCAL) return 1.0f / x;
    else if constexpr (OP == RTEN_HIP_UNARY_EXP) return vm::exp_full(x);
    else if constexpr (OP == RTEN_HIP_UNARY_LOG) return (float)log((double)x);
    else { // Softplus: exp(x).ln_1p() with the intermediate rounded to f32
        const float e = (float)exp((double)x);
        return (float)log1p((double)e);
    }
}

// No __restrict__: y may equal x (each element is read before it is written, by the same lane).  `head` = scalar elements before the first
// 16-byte boundary (the same for x and y), or -1: no vector body.
template <int OP>
__global__ __launch_bounds__(MATH_THREADS) void unary_math_kernel(int64_t n, const float *x, float *y, int head) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (head < 0) {
        for (int64_t i = tid; i < n; i += stride) y[i] = unary_math<OP>(x[i]);
        return;
    }
    const int64_t n4 = (n - head) >> 2;
    const f32x4 *xv = reinterpret_cast<const f32x4 *>(x + head);
    f32x4 *yv = reinterpret_cast<f32x4 *>(y + head);
    for (int64_t i = tid; i < n4; i += stride) {
        const f32x4 v = xv[i];
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = unary_math<OP>(v[k]);
        yv[i] = r;
    }
    if (tid < head) y[tid] = unary_math<OP>(x[tid]);
    for (int64_t i = head + (n4 << 2) + tid; i < n; i += stride) y[i] = unary_math<OP>(x[i]);
}

} // namespace

RTEN_EXPORT int32_t rten_hip_unary_f32(rten_hip_ctx *ctx, int32_t op, int64_t n, const float *x, float *y) {
    RTEN_CHECK_CTX(ctx);
    if (op < RTEN_HIP_UNARY_NEG || op > RTEN_HIP_UNARY_SOFTPLUS) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "unary: unknown operator code");
    if (n < 0) return RTEN_HIP_ERR_INVALID_VALUE;
    if (n == 0) return RTEN_HIP_OK;
    if (!x || !y) return RTEN_HIP_ERR_INVALID_VALUE;
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
    int head = -1;
    if (((xa ^ ya) & 15u) == 0 && (xa & 3u) == 0) {
        head = (int)(((16u - (xa & 15u)) & 15u) >> 2);
        if (n - head < 4) head = -1;
    }
    const dim3 grid(math_blocks(head < 0 ? n : (n - head) / 4)), block(MATH_THREADS);
    ProfScope ps(ctx, "unary_f32", 0.0, 8.0 * n);
    switch (op) {
#define RTEN_UNARY_CASE(K) case K: hipLaunchKernelGGL((unary_math_kernel<K>), grid, block, 0, ctx->stream, n, x, y, head); break;
    RTEN_UNARY_CASE(RTEN_HIP_UNARY_NEG) RTEN_UNARY_CASE(RTEN_HIP_UNARY_ABS) RTEN_UNARY_CASE(RTEN_HIP_UNARY_SIGN) RTEN_UNARY_CASE(RTEN_HIP_UNARY_FLOOR)
    RTEN_UNARY_CASE(RTEN_HIP_UNARY_CEIL) RTEN_UNARY_CASE(RTEN_HIP_UNARY_ROUND) RTEN_UNARY_CASE(RTEN_HIP_UNARY_SQRT) RTEN_UNARY_CASE(RTEN_HIP_UNARY_RECIPROCAL)
    RTEN_UNARY_CASE(RTEN_HIP_UNARY_EXP) RTEN_UNARY_CASE(RTEN_HIP_UNARY_LOG) RTEN_UNARY_CASE(RTEN_HIP_UNARY_SOFTPLUS)
#undef RTEN_UNARY_CASE
    }
    RTEN_LAUNCH_CHECK(ctx, "unary_f32");
    return RTEN_HIP_OK;
}
