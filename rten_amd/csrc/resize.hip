// Resize / Upsample (src/ops/resize.rs:48-243): nearest and bilinear resampling of `planes` f32 planes of in_h x in_w into
// out_h x out_w (the NCHW form every supported rank is reshaped to, resize.rs:334-408).
//
// Every rounded f32 operation of the reference is restated one at a time (input_coord, the f32::clamp to [0, len - 1], the
// `as usize` casts, the nearest-mode roundings, lerp as three roundings, x first then y), so results are bit-identical.
//
// Layout (HBM-bound): a workgroup owns one output row `oy` of a chunk of planes.  The row's source coordinate is computed once
// per workgroup, a thread's VEC column coordinates once per column group, and both are reused for every plane of the chunk.
// A thread writes VEC consecutive outputs with one store: VEC = 4 when the output width is a multiple of 4 (every row then
// starts 16-byte aligned), 2 when it is even, 1 otherwise (lanes then cover consecutive columns: 256 B per wave store).
#include "internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int RS_THREADS = 256;

struct ResizeArgs {
    int64_t planes, in_h, in_w, out_h, out_w;
    float inv_y, inv_x;
    int32_t coord, nearest;
    int32_t cols;    // column groups per output row (out_w / VEC)
    int32_t tw, pr;  // threads per plane row (<= RS_THREADS), plane rows per workgroup
    int64_t chunk;   // planes per workgroup (a multiple of pr)
    int64_t blocks;  // out_h * ceil(planes / chunk)
};

// input_coord (resize.rs:48-75); `d as f32` and `(len - 1) as f32` round to nearest like Rust's `as`
__device__ __forceinline__ float input_coord(int64_t d, float s, int32_t mode, int64_t len_in, int64_t len_out) {
    const float df = (float)d;
    switch (mode) {
    case RTEN_HIP_RESIZE_COORD_ASYMMETRIC: return s * df;
    case RTEN_HIP_RESIZE_COORD_ALIGN_CORNERS: return df * (float)(len_in - 1) / (float)(len_out - 1); // length 1: 0 / 0 = NaN, as in the reference
    case RTEN_HIP_RESIZE_COORD_PYTORCH_HALF_PIXEL: return len_out > 1 ? s * (df + 0.5f) - 0.5f : 0.f;
    default: return s * (df + 0.5f) - 0.5f; // half_pixel
    }
}

// f32::clamp(c, 0, len as f32 - 1): NaN stays NaN
__device__ __forceinline__ float clamp_coord(float c, int64_t len) {
    const float hi = (float)len - 1.f;
    if (c < 0.f) c = 0.f;
    if (c > hi) c = hi;
    return c;
}

// `c as usize` of a clamped coordinate (saturating: NaN -> 0).  The min() only matters past 2^24, where `len as f32 - 1` can round
// above len - 1 (the reference's index would panic there): it keeps every read in bounds.
__device__ __forceinline__ int64_t to_index(float c, int64_t len) {
    const int64_t i = c == c ? (int64_t)c : 0;
    return i < len - 1 ? i : len - 1;
}

// round_coord of nearest_resize (resize.rs:121-141); Floor is the truncating cast itself
__device__ __forceinline__ int64_t nearest_index(int64_t d, float s, const ResizeArgs &a, int64_t len_in, int64_t len_out) {
    const float c = clamp_coord(input_coord(d, s, a.coord, len_in, len_out), len_in);
    float r;
    switch (a.nearest) {
    case RTEN_HIP_RESIZE_NEAREST_CEIL: r = ceilf(c); break;
    case RTEN_HIP_RESIZE_NEAREST_FLOOR: r = c; break;
    case RTEN_HIP_RESIZE_NEAREST_ROUND_PREFER_CEIL: r = c - truncf(c) == 0.5f ? ceilf(c) : roundf(c); break;
    default: r = c - truncf(c) == 0.5f ? floorf(c) : roundf(c); break; // round_prefer_floor; roundf rounds half away from zero like f32::round
    }
    return to_index(r, len_in);
}

struct Tap {
    int64_t i1, i2;
    float w;
};
// bilinear_resize (resize.rs:191-202): i1 = c as usize, i2 = min(i1 + 1, len - 1), w = c - i1 as f32
__device__ __forceinline__ Tap linear_tap(int64_t d, float s, int32_t mode, int64_t len_in, int64_t len_out) {
    const float c = clamp_coord(input_coord(d, s, mode, len_in, len_out), len_in);
    Tap t;
    t.i1 = to_index(c, len_in);
    t.i2 = t.i1 + 1 < len_in - 1 ? t.i1 + 1 : len_in - 1;
    t.w = c - (float)t.i1;
    return t;
}

// lerp (resize.rs:102-104): three roundings (the library is built with -ffp-contract=off)
__device__ __forceinline__ float lerp(float a, float b, float w) { return (1.f - w) * a + w * b; }

template <int VEC>
__device__ __forceinline__ void store_vec(float *p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<f32x4 *>(p) = f32x4{v[0], v[1], v[2], v[3]};
    else if constexpr (VEC == 2) *reinterpret_cast<f32x2 *>(p) = f32x2{v[0], v[1]};
    else *p = v[0];
}

template <int VEC, bool LINEAR>
__global__ __launch_bounds__(RS_THREADS) void resize_kernel(ResizeArgs a, const float *__restrict__ x, float *__restrict__ y) {
    const int tx = (int)threadIdx.x % a.tw, ty = (int)threadIdx.x / a.tw;
    if (ty >= a.pr) return;
    const int64_t in_plane = a.in_h * a.in_w, out_plane = a.out_h * a.out_w;
    for (int64_t blk = blockIdx.x; blk < a.blocks; blk += gridDim.x) {
        const int64_t oy = blk % a.out_h, p0 = (blk / a.out_h) * a.chunk;
        const int64_t p1 = p0 + a.chunk < a.planes ? p0 + a.chunk : a.planes;
        if constexpr (LINEAR) {
            const Tap row = linear_tap(oy, a.inv_y, a.coord, a.in_h, a.out_h);
            for (int32_t cg = tx; cg < a.cols; cg += a.tw) {
                int64_t x1[VEC], x2[VEC];
                float wx[VEC];
#pragma unroll
                for (int k = 0; k < VEC; k++) {
                    const Tap t = linear_tap((int64_t)cg * VEC + k, a.inv_x, a.coord, a.in_w, a.out_w);
                    x1[k] = t.i1; x2[k] = t.i2; wx[k] = t.w;
                }
                for (int64_t p = p0 + ty; p < p1; p += a.pr) {
                    const float *r1 = x + p * in_plane + row.i1 * a.in_w, *r2 = x + p * in_plane + row.i2 * a.in_w;
                    float v[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; k++) {
                        const float top = lerp(r1[x1[k]], r1[x2[k]], wx[k]);
                        const float bottom = lerp(r2[x1[k]], r2[x2[k]], wx[k]);
                        v[k] = lerp(top, bottom, row.w);
                    }
                    store_vec<VEC>(y + p * out_plane + oy * a.out_w + (int64_t)cg * VEC, v);
                }
            }
        } else {
            const int64_t iy = nearest_index(oy, a.inv_y, a, a.in_h, a.out_h);
            for (int32_t cg = tx; cg < a.cols; cg += a.tw) {
                int64_t ix[VEC];
#pragma unroll
                for (int k = 0; k < VEC; k++) ix[k] = nearest_index((int64_t)cg * VEC + k, a.inv_x, a, a.in_w, a.out_w);
                for (int64_t p = p0 + ty; p < p1; p += a.pr) {
                    const float *r = x + p * in_plane + iy * a.in_w;
                    float v[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; k++) v[k] = r[ix[k]];
                    store_vec<VEC>(y + p * out_plane + oy * a.out_w + (int64_t)cg * VEC, v);
                }
            }
        }
    }
}

template <int VEC>
void launch(const ResizeArgs &a, bool linear, dim3 grid, hipStream_t s, const float *x, float *y) {
    if (linear) hipLaunchKernelGGL((resize_kernel<VEC, true>), grid, dim3(RS_THREADS), 0, s, a, x, y);
    else hipLaunchKernelGGL((resize_kernel<VEC, false>), grid, dim3(RS_THREADS), 0, s, a, x, y);
}

} // namespace

RTEN_EXPORT int32_t rten_hip_resize_f32(rten_hip_ctx *ctx, int32_t mode, int32_t coord_mode, int32_t nearest_mode, int64_t planes, int64_t in_h, int64_t in_w,
                                        int64_t out_h, int64_t out_w, float inv_scale_y, float inv_scale_x, const float *x, float *y) {
    RTEN_CHECK_CTX(ctx);
    if (mode != RTEN_HIP_RESIZE_MODE_NEAREST && mode != RTEN_HIP_RESIZE_MODE_LINEAR)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "resize: unknown mode");
    if (coord_mode < RTEN_HIP_RESIZE_COORD_HALF_PIXEL || coord_mode > RTEN_HIP_RESIZE_COORD_PYTORCH_HALF_PIXEL)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "resize: unknown coordinate transformation mode");
    if (nearest_mode < RTEN_HIP_RESIZE_NEAREST_ROUND_PREFER_FLOOR || nearest_mode > RTEN_HIP_RESIZE_NEAREST_CEIL)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "resize: unknown nearest mode");
    const int64_t lim = 0x7fffffff;
    if (planes < 0 || in_h < 0 || in_w < 0 || out_h < 0 || out_w < 0 || planes > lim || in_h > lim || in_w > lim || out_h > lim || out_w > lim)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "resize: bad dimension");
    if (planes == 0 || out_h == 0 || out_w == 0) return RTEN_HIP_OK;
    if (in_h == 0 || in_w == 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "resize: an empty input cannot give a non-empty output");
    if (!x || !y) return RTEN_HIP_ERR_INVALID_VALUE;
    const uintptr_t yp = (uintptr_t)y;
    const int vec = (out_w % 4 == 0 && (yp & 15u) == 0) ? 4 : (out_w % 2 == 0 && (yp & 7u) == 0) ? 2 : 1;
    ResizeArgs a;
    a.planes = planes; a.in_h = in_h; a.in_w = in_w; a.out_h = out_h; a.out_w = out_w;
    a.inv_y = inv_scale_y; a.inv_x = inv_scale_x;
    a.coord = coord_mode; a.nearest = nearest_mode;
    a.cols = (int32_t)(out_w / vec);
    a.tw = a.cols < RS_THREADS ? a.cols : RS_THREADS;
    a.pr = RS_THREADS / a.tw;
    // about 8192 workgroups of one output row each; a thread then stores up to 16 vectors per column group
    int64_t k = ceil_div64(planes * out_h, (int64_t)a.pr * 8192);
    if (k < 1) k = 1;
    if (k > 16) k = 16;
    a.chunk = (int64_t)a.pr * k;
    a.blocks = out_h * ceil_div64(planes, a.chunk);
    const dim3 grid((unsigned)(a.blocks < 65536 ? a.blocks : 65536));
    const bool linear = mode == RTEN_HIP_RESIZE_MODE_LINEAR;
    ProfScope ps(ctx, "resize_f32", 0.0, 4.0 * ((double)planes * out_h * out_w + (double)planes * in_h * in_w));
    if (vec == 4) launch<4>(a, linear, grid, ctx->stream, x, y);
    else if (vec == 2) launch<2>(a, linear, grid, ctx->stream, x, y);
    else launch<1>(a, linear, grid, ctx->stream, x, y);
    RTEN_LAUNCH_CHECK(ctx, "resize_f32");
    return RTEN_HIP_OK;
}
