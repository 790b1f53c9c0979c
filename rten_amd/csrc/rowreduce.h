// The order-defining helpers of the wave-per-row reductions (rowwise.hip, norm.hip): a 64-lane wavefront is four 16-lane
// AVX-512 vectors side by side, so lane t = 16u + l is accumulator slot (u, l) of the reference's fold_unroll<4>
// (rten-simd/src/iter.rs:97-120, rten-vecmath/src/sum.rs:27-33,110-127).
#pragma once
#include <hip/hip_runtime.h>

#include "vecmath.h"

static __device__ __forceinline__ float lane_bcast(float v, int src_lane) { return __shfl(v, src_lane, 64); }

// fold_unroll<4> order (sum.rs:27-33,60-66,86-92,110-127).  kind 0: sum x ; kind 1: sum (x-off)^2 via mul_add (off = 0: SumSquare) ; kind 2: sum |x|.
// `get(i)` returns element i (i < n).  All lanes return the same total.
// BATCH > 1: the chain of adds is unchanged (one accumulator per lane, chunks in order), but BATCH chunks are requested before the first of them is
// added -- for a `get` that reads memory, a load per add is one round trip per 256 bytes.
template <int KIND, int BATCH = 1, typename Get, typename Index>
__device__ __forceinline__ float simd16_reduce(Get get, Index n, float off, int lane) {
    auto f = [&](float acc, float x) -> float {
        if constexpr (KIND == 0) return acc + x;
        else if constexpr (KIND == 1) { const float d = x - off; return vm::fma(d, d, acc); }
        else return acc + __builtin_fabsf(x);
    };
    float acc = 0.f;
    const Index full4 = n / 64;
    Index c = 0;
    if constexpr (BATCH > 1) {
        for (; c + BATCH <= full4; c += BATCH) {
            float t[BATCH];
#pragma unroll
            for (int k = 0; k < BATCH; k++) t[k] = get((c + k) * 64 + lane);
#pragma unroll
            for (int k = 0; k < BATCH; k++) acc = f(acc, t[k]);
        }
    }
    for (; c < full4; c++) acc = f(acc, get(c * 64 + lane));
    // acc0 += acc1; += acc2; += acc3  (lanes 0..15 hold the running vector)
    float a = acc;
    a = a + lane_bcast(acc, (lane & 15) + 16);
    a = a + lane_bcast(acc, (lane & 15) + 32);
    a = a + lane_bcast(acc, (lane & 15) + 48);
    Index i0 = full4 * 64;
    const int l = lane & 15;
    for (; i0 + 16 <= n; i0 += 16) a = f(a, get(i0 + l));
    if (i0 + l < n) a = f(a, get(i0 + l)); // masked tail: other lanes keep their value
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k++) s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), k));
    return s;
}
