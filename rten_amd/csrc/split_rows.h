// The two row-wise stages that the split decode forms share (gqa_split.hip, attention_split.hip), lifted from gqa_split.hip's softmax and fold kernels
// unchanged: each is the body of a thin kernel that works out its row, its length and where the result goes.
#pragma once
#include "internal.h"
#include "vecmath.h"

namespace {

constexpr int SM_THREADS = 1024, SM_TILE = 4096;
constexpr int FOLD_COLS = 32, FOLD_TILE = 128;

// One workgroup of SM_THREADS threads: the softmax of rowwise.hip (softmax_long_kernel) on the score row x[0, len) in scratch, up to the division: e over
// x, 1 / sum to *inv_out.  The maximum from f32::MIN (order-free); e = exp_reduced(x - max) for SM_TILE elements at a time, written back over x and into an
// LDS tile; 16 lanes of wave 0 run the 16 ordered chains over the tile (chain l adds the elements i = l mod 16 in index order) while the other waves fill
// the second tile; lanes 0..15 added from lane 0.
__device__ __forceinline__ void split_softmax_row(float *x, int len, float *inv_out) {
    __shared__ float tile[2][SM_TILE];
    __shared__ float red[SM_THREADS / 64];
    const int tid = threadIdx.x;
    float mx = -3.40282347e+38f; // f32::MIN (softmax.rs:181)
    for (int i = tid; i < len; i += SM_THREADS) mx = fmaxf(mx, x[i]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SM_THREADS / 64; w++) mx = fmaxf(mx, red[w]);
    float a = 0.f;
    for (int t0 = 0, it = 0; t0 < len; t0 += SM_TILE, it++) {
        float *buf = tile[it & 1];
        float xv[SM_TILE / SM_THREADS];
#pragma unroll
        for (int j = 0; j < SM_TILE / SM_THREADS; j++) {
            const int i = t0 + j * SM_THREADS + tid;
            xv[j] = i < len ? x[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < SM_TILE / SM_THREADS; j++) {
            const int i = t0 + j * SM_THREADS + tid;
            if (i < len) {
                const float e = vm::exp_reduced(xv[j] - mx);
                x[i] = e;
                buf[j * SM_THREADS + tid] = e;
            }
        }
        __syncthreads();
        // the 16 ordered chains; the other waves go on to fill the other tile, and meet this wave again at the next barrier before they come back to this one
        if (tid < 16) {
            const int n = len - t0 < SM_TILE ? len - t0 : SM_TILE;
            int i = tid;
            for (; i + 16 * 7 < n; i += 16 * 8) { // eight reads in flight, then the eight adds in index order
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; j++) v[j] = buf[i + 16 * j];
#pragma unroll
                for (int j = 0; j < 8; j++) a = a + v[j];
            }
            for (; i < n; i += 16) a = a + buf[i];
        }
    }
    if (tid < 64) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < 16; k++) sum = sum + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), k));
        if (tid == 0) *inv_out = 1.0f / sum;
    }
}

// One workgroup of 256 threads: FOLD_COLS output columns of one row.  src = the row's block sums [nblk, D] at the first of those columns (16-byte
// aligned), dst = the output row at the same column.  FOLD_TILE blocks x FOLD_COLS columns are staged into LDS with 16-byte loads (the next tile is in
// flight while this one is folded), and FOLD_COLS threads fold them in block order: block 0 stored, the rest added left to right.
__device__ __forceinline__ void split_fold_row(const float *src, int nblk, int D, float *dst) {
    __shared__ float4 tile[FOLD_TILE][FOLD_COLS / 4];
    const int tid = threadIdx.x;
    const int rr = tid >> 3, c4 = tid & 7;
    float4 reg[4];
    auto load = [&](int b0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int blk = b0 + rr + 32 * i;
            reg[i] = blk < nblk ? *reinterpret_cast<const float4 *>(src + (int64_t)blk * D + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    load(0);
    float o = 0.f;
    for (int b0 = 0; b0 < nblk; b0 += FOLD_TILE) {
#pragma unroll
        for (int i = 0; i < 4; i++) tile[rr + 32 * i][c4] = reg[i];
        __syncthreads();
        if (b0 + FOLD_TILE < nblk) load(b0 + FOLD_TILE);
        if (tid < FOLD_COLS) {
            const float *tf = reinterpret_cast<const float *>(&tile[0][0]);
            const int cnt = nblk - b0 < FOLD_TILE ? nblk - b0 : FOLD_TILE;
            int j = 0;
            if (b0 == 0) o = tf[tid], j = 1; // the first block is stored, the rest are added
            for (; j + 7 < cnt; j += 8) {
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = tf[(j + i) * FOLD_COLS + tid];
#pragma unroll
                for (int i = 0; i < 8; i++) o = o + v[i];
            }
            for (; j < cnt; j++) o = o + tf[j * FOLD_COLS + tid];
        }
        __syncthreads();
    }
    if (tid < FOLD_COLS) dst[tid] = o;
}

} // namespace
