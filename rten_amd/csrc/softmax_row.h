// The row softmax that the attention units share (gqa.hip, attention_kv.hip): moved here from gqa.hip unchanged.
#pragma once
#include "rowreduce.h"
#include "vecmath.h"

namespace {

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

} // namespace
