// GridSample (src/ops/grid_sample.rs:12-125): bilinear sampling of x [batch, channels, in_h, in_w] at the normalised coordinates of
// grid [batch, out_h, out_w, 2], zero padding, into y [batch, channels, out_h, out_w].
//
// Every rounded f32 operation of the reference is restated one at a time (the library is built with -ffp-contract=off): the scaling of the
// coordinate, floor, the lerp weight, Rust's `as i32` of the floor, lerp as `a + (b - a) * w`, x first then y.  Results are bit-identical.
//
// Layout (gather- and store-bound): a thread owns ONE output pixel of one batch row and a tile of GS_CTILE_* channels.  Its coordinates, the
// four tap offsets and their in-bounds masks are computed once and reused for every channel of the tile.  Adjacent lanes own adjacent pixels
// of the flattened out_h x out_w plane, so the 8-byte grid load and every store are contiguous across a wave (512 B / 256 B).  Pixel tiles
// (times the batch) are grid dimension x, channel tiles grid dimension y; both are walked with a stride, so no shape exceeds a grid cap.
// The tile is chosen on the host (pick_ctile): the largest of 16 / 4 / 1 that still leaves GS_MIN_BLOCKS workgroups.
#include "internal.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int GS_THREADS = 256;
constexpr int GS_CTILE_LARGE = 16, GS_CTILE_SMALL = 4; // channels per thread; below GS_MIN_BLOCKS workgroups even at 4: one channel per thread
constexpr int64_t GS_MIN_BLOCKS = 1024;                // 4 workgroups of 256 threads on each of the 256 CUs
constexpr int64_t GS_MAX_GRID_X = (1 << 24) - 1, GS_MAX_GRID_Y = 65535; // x: blocks * GS_THREADS stays below 2^32, the runtime's limit on a dimension's threads

struct GridSampleArgs {
    int64_t channels, in_h, in_w, out_plane;
    int64_t pix_tiles; // ceil(out_plane / GS_THREADS)
    int64_t blocks;    // batch * pix_tiles
    int64_t ctiles;    // ceil(channels / ctile)
    int32_t ctile, align_corners, grid8; // grid8: the grid pointer is 8-byte aligned (one load per coordinate pair)
};

// Rust's `f as i32`: truncation toward zero, saturating at the ends of the range, NaN -> 0
__device__ __forceinline__ int32_t rust_f32_as_i32(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.f) return 2147483647;
    if (f <= -2147483648.f) return -2147483647 - 1;
    return (int32_t)f;
}

struct Axis {
    int64_t i0, i1; // floor(s) as i32 and its neighbour (a 64-bit sum: past i32::MAX it is out of bounds, as the reference's wrapped value is)
    float w;        // s - floor(s)
};
// grid_sample.rs:59-93 for one axis
__device__ __forceinline__ Axis sample_axis(float g, int64_t len, int32_t align_corners) {
    const float u = (g + 1.f) * 0.5f;
    float s;
    if (align_corners) s = ((float)len - 1.f) * u;
    else s = (float)len * u - 0.5f;
    const float fl = floorf(s);
    Axis a;
    a.w = s - fl;
    a.i0 = rust_f32_as_i32(fl);
    a.i1 = a.i0 + 1;
    return a;
}

// lerp (grid_sample.rs:13-15): three roundings
__device__ __forceinline__ float lerp(float a, float b, float w) { return a + (b - a) * w; }

__global__ __launch_bounds__(GS_THREADS) void grid_sample_kernel(GridSampleArgs a, const float *__restrict__ x, const float *__restrict__ grid, float *__restrict__ y) {
    const int64_t in_plane = a.in_h * a.in_w;
    for (int64_t blk = blockIdx.x; blk < a.blocks; blk += gridDim.x) {
        const int64_t n = blk / a.pix_tiles, p = (blk % a.pix_tiles) * GS_THREADS + threadIdx.x;
        if (p >= a.out_plane) continue;
        const float *g = grid + (n * a.out_plane + p) * 2;
        float g0, g1;
        if (a.grid8) {
            const f32x2 v = *reinterpret_cast<const f32x2 *>(g);
            g0 = v.x; g1 = v.y;
        } else {
            g0 = g[0]; g1 = g[1];
        }
        const Axis ax = sample_axis(g0, a.in_w, a.align_corners), ay = sample_axis(g1, a.in_h, a.align_corners);
        const bool x0 = ax.i0 >= 0 && ax.i0 < a.in_w, x1 = ax.i1 >= 0 && ax.i1 < a.in_w;
        const bool y0 = ay.i0 >= 0 && ay.i0 < a.in_h, y1 = ay.i1 >= 0 && ay.i1 < a.in_h;
        const bool m00 = y0 && x0, m01 = y0 && x1, m10 = y1 && x0, m11 = y1 && x1;
        // a tap outside the plane reads pixel 0 of the plane instead (the plane is not empty) and the value is dropped: no address outside
        // x is formed into a load, and what pixel 0 holds -- a NaN, say -- does not reach the output
        const int64_t o00 = m00 ? ay.i0 * a.in_w + ax.i0 : 0, o01 = m01 ? ay.i0 * a.in_w + ax.i1 : 0;
        const int64_t o10 = m10 ? ay.i1 * a.in_w + ax.i0 : 0, o11 = m11 ? ay.i1 * a.in_w + ax.i1 : 0;
        const float *xn = x + n * a.channels * in_plane;
        float *yn = y + n * a.channels * a.out_plane + p;
        for (int64_t ct = blockIdx.y; ct < a.ctiles; ct += gridDim.y) {
            const int64_t c0 = ct * a.ctile, c1 = c0 + a.ctile < a.channels ? c0 + a.ctile : a.channels;
#pragma unroll 4
            for (int64_t c = c0; c < c1; c++) {
                const float *xc = xn + c * in_plane;
                const float v00 = xc[o00], v01 = xc[o01], v10 = xc[o10], v11 = xc[o11];
                const float p00 = m00 ? v00 : 0.f, p01 = m01 ? v01 : 0.f, p10 = m10 ? v10 : 0.f, p11 = m11 ? v11 : 0.f;
                const float top = lerp(p00, p01, ax.w), bottom = lerp(p10, p11, ax.w);
                yn[c * a.out_plane] = lerp(top, bottom, ay.w);
            }
        }
    }
}

// Channels per thread.  A large tile amortises the coordinate arithmetic (about 40 VALU operations and the grid load against 4 loads, 9
// operations and a store per channel) and keeps 4 * tile independent loads in flight per thread; but the launch must still fill the chip,
// and small planes with many channels (deformable attention: 100 x 4 points, 32 channels, 64 batch rows) only do so through their channels.
int32_t pick_ctile(int64_t channels, int64_t pixel_blocks) {
    for (int32_t t : {GS_CTILE_LARGE, GS_CTILE_SMALL})
        if (pixel_blocks * ceil_div64(channels, t) >= GS_MIN_BLOCKS) return t;
    return 1;
}

} // namespace

RTEN_EXPORT int32_t rten_hip_grid_sample_f32(rten_hip_ctx *ctx, int32_t align_corners, int64_t batch, int64_t channels, int64_t in_h, int64_t in_w, int64_t out_h,
                                             int64_t out_w, const float *x, const float *grid, float *y) {
    RTEN_CHECK_CTX(ctx);
    const int64_t lim = 0x7fffffff;
    if (batch < 0 || channels < 0 || in_h < 0 || in_w < 0 || out_h < 0 || out_w < 0 || batch > lim || channels > lim || in_h > lim || in_w > lim || out_h > lim || out_w > lim)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "grid_sample: bad dimension");
    if (batch == 0 || channels == 0 || out_h == 0 || out_w == 0) return RTEN_HIP_OK;
    const int64_t out_plane = out_h * out_w;
    if (!y) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "grid_sample: null output");
    if (in_h == 0 || in_w == 0) { // every coordinate is out of bounds (grid_sample.rs:40-43)
        RTEN_HIP_TRY(ctx, hipMemsetAsync(y, 0, sizeof(float) * (size_t)(batch * channels * out_plane), ctx->stream));
        return RTEN_HIP_OK;
    }
    if (!x || !grid) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "grid_sample: null input or grid");
    GridSampleArgs a;
    a.channels = channels; a.in_h = in_h; a.in_w = in_w; a.out_plane = out_plane;
    a.pix_tiles = ceil_div64(out_plane, GS_THREADS);
    a.blocks = batch * a.pix_tiles;
    a.ctile = pick_ctile(channels, a.blocks);
    a.ctiles = ceil_div64(channels, a.ctile);
    a.align_corners = align_corners != 0;
    a.grid8 = ((uintptr_t)grid & 7u) == 0;
    const dim3 launch_grid((unsigned)(a.blocks < GS_MAX_GRID_X ? a.blocks : GS_MAX_GRID_X), (unsigned)(a.ctiles < GS_MAX_GRID_Y ? a.ctiles : GS_MAX_GRID_Y));
    ProfScope ps(ctx, "grid_sample_f32", 0.0, 4.0 * ((double)batch * channels * (out_plane + in_h * in_w) + 2.0 * batch * out_plane));
    hipLaunchKernelGGL(grid_sample_kernel, launch_grid, dim3(GS_THREADS), 0, ctx->stream, a, x, grid, y);
    RTEN_LAUNCH_CHECK(ctx, "grid_sample_f32");
    return RTEN_HIP_OK;
}
