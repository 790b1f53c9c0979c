// Pad (src/ops/pad.rs) of 4-byte elements: one launch, a gather over the output.  Each output element decomposes its flat index over the (merged) axes,
// maps every coordinate to a source coordinate by the mode's formula (pad.rs:235-286: ReflectPad / EdgePad / WrapPad::src_index, constant mode: the
// non-pad region of pad.rs:86-106) and reads one word, or takes the fill word where a constant-mode coordinate falls outside.
//
// Layout: one output word per thread-iteration, consecutive lanes along the innermost axis (coalesced stores; loads coalesced wherever the innermost
// axis runs forward, which is everywhere except inside a reflected border).  Adjacent axes that are neither padded nor cropped are merged on the host
// (N and C of an NCHW spatial pad become one axis: one division fewer per element).  When the innermost axis is unpadded and x, y, its length and its crop
// are multiples of 16 bytes, the same kernel runs on 16-byte words.  Indices are 32-bit whenever both tensors have fewer than 2^31 words.
#include "internal.h"

namespace {

constexpr int PAD_THREADS = 256;

struct PadArgs {
    int32_t ndim, mode;
    uint32_t fill;
    int64_t n;            // output words
    int64_t out[6];       // output extent per axis
    int64_t len[6];       // cropped source extent per axis
    int64_t pad[6];       // begin pad (>= 0) per axis
    int64_t stride[6];    // source stride per axis, in words
    int64_t base;         // source offset of the cropped region's first word
};

template <typename I>
__device__ __forceinline__ I pad_src_index(int mode, I o, I len, I p) {
    if (mode == RTEN_HIP_PAD_REFLECT) {
        I s = o < p ? p - o : (o < len + p ? o - p : len - (o - len - p) - 2);
        s %= len; // rem_euclid
        return s < 0 ? s + len : s;
    }
    if (mode == RTEN_HIP_PAD_EDGE) {
        const I s = o - p;
        return s < 0 ? 0 : (s > len - 1 ? len - 1 : s);
    }
    I s = (o - p) % len; // wrap
    return s < 0 ? s + len : s;
}

template <typename T>
__device__ __forceinline__ T pad_fill_word(uint32_t bits);
template <>
__device__ __forceinline__ uint32_t pad_fill_word<uint32_t>(uint32_t bits) { return bits; }
template <>
__device__ __forceinline__ uint4 pad_fill_word<uint4>(uint32_t bits) { return make_uint4(bits, bits, bits, bits); }

// T = the word moved (4 or 16 bytes), I = index type (int32_t when every offset fits, else int64_t)
template <typename T, typename I>
__global__ __launch_bounds__(PAD_THREADS) void pad_kernel(const PadArgs p, const T *__restrict__ x, T *__restrict__ y) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += step) {
        I r = (I)i, off = (I)p.base;
        bool inside = true;
        for (int d = p.ndim - 1; d >= 0; d--) {
            const I extent = (I)p.out[d], len = (I)p.len[d], pb = (I)p.pad[d];
            const I q = r / extent, o = r - q * extent;
            r = q;
            I s;
            if (p.mode == RTEN_HIP_PAD_CONSTANT || extent == len) {
                s = o - pb;
                const bool in_axis = s >= 0 && s < len;
                inside = inside && in_axis;
                s = in_axis ? s : 0; // (the offset stays inside x even where it is not read)
            } else {
                s = pad_src_index<I>(p.mode, o, len, pb);
            }
            off += s * (I)p.stride[d];
        }
        y[i] = inside ? x[off] : pad_fill_word<T>(p.fill);
    }
}

template <typename T, typename I>
void pad_launch(rten_hip_ctx *ctx, const PadArgs &p, const void *x, void *y) {
    int64_t b = (p.n + PAD_THREADS - 1) / PAD_THREADS;
    if (b > 2048) b = 2048;
    hipLaunchKernelGGL((pad_kernel<T, I>), dim3((unsigned)b), dim3(PAD_THREADS), 0, ctx->stream, p, (const T *)x, (T *)y);
}

} // namespace

RTEN_EXPORT int32_t rten_hip_pad_b32(rten_hip_ctx *ctx, int32_t mode, int32_t ndim, const int64_t *x_shape, const int64_t *pads, uint32_t fill_bits, const void *x,
                                     void *y) {
    RTEN_CHECK_CTX(ctx);
    if (mode < RTEN_HIP_PAD_CONSTANT || mode > RTEN_HIP_PAD_WRAP || ndim < 0 || ndim > 6 || (ndim && (!x_shape || !pads)))
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "pad: unknown mode / more than 6 dims");
    int64_t out[6], len[6], pb[6], crop[6], xs[6], x_words = 1, n = 1;
    bool padded[6];
    const int64_t lim = 0x7fffffff;
    for (int d = 0; d < ndim; d++) {
        const int64_t b = pads[d], e = pads[ndim + d];
        if (x_shape[d] < 0 || x_shape[d] > lim || b < -lim || b > lim || e < -lim || e > lim) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "pad: bad dimension");
        crop[d] = b < 0 ? -b : 0;
        const int64_t crop_e = e < 0 ? -e : 0;
        if (crop[d] + crop_e > x_shape[d]) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "Negative pads remove more elements than axis contains");
        len[d] = x_shape[d] - crop[d] - crop_e;
        pb[d] = b > 0 ? b : 0;
        out[d] = pb[d] + len[d] + (e > 0 ? e : 0);
        if (out[d] > lim) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "pad: bad dimension");
        padded[d] = b != 0 || e != 0;
        n *= out[d];
        x_words *= x_shape[d];
    }
    for (int d = 0; d < ndim; d++) // (every source index formula divides by len: the reference's check, pad.rs:120-124)
        if (mode != RTEN_HIP_PAD_CONSTANT && out[d] != len[d] && len[d] == 0 && n != 0)
            return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "Padded dimension for non-constant padding is empty");
    if (n == 0) return RTEN_HIP_OK;
    if (!y || (!x && x_words != 0)) return RTEN_HIP_ERR_INVALID_VALUE; // (an empty x is never read: constant mode fills)
    int64_t acc = 1;
    for (int d = ndim - 1; d >= 0; d--) { xs[d] = acc; acc *= x_shape[d]; }

    // 16-byte words along an innermost axis that is only copied (cropped by whole words at most)
    int vec = 1;
    if (ndim > 0) {
        const int l = ndim - 1;
        const bool al = (((uintptr_t)x | (uintptr_t)y) & 15u) == 0;
        if (al && out[l] == len[l] && len[l] % 4 == 0 && crop[l] % 4 == 0 && x_shape[l] % 4 == 0) vec = 4;
    }
    PadArgs p = {};
    p.mode = mode;
    p.fill = fill_bits;
    p.n = n / vec;
    p.base = 0;
    // merge runs of untouched axes (no pad, no crop): their words are contiguous in both tensors
    int m = 0;
    for (int d = 0; d < ndim; d++) {
        const int64_t o = d == ndim - 1 ? out[d] / vec : out[d], ln = d == ndim - 1 ? len[d] / vec : len[d];
        const int64_t st = d == ndim - 1 ? 1 : xs[d] / vec, cr = d == ndim - 1 ? crop[d] / vec : crop[d];
        p.base += cr * st;
        if (m > 0 && !padded[d] && !padded[d - 1]) {
            p.out[m - 1] *= o; p.len[m - 1] *= ln; p.stride[m - 1] = st;
        } else {
            p.out[m] = o; p.len[m] = ln; p.pad[m] = pb[d]; p.stride[m] = st;
            m++;
        }
    }
    p.ndim = m;
    const bool small = n < lim && x_words < lim;
    ProfScope ps(ctx, "pad_b32", 0.0, 8.0 * n);
    if (vec == 4) {
        if (small) pad_launch<uint4, int32_t>(ctx, p, x, y);
        else pad_launch<uint4, int64_t>(ctx, p, x, y);
    } else {
        if (small) pad_launch<uint32_t, int32_t>(ctx, p, x, y);
        else pad_launch<uint32_t, int64_t>(ctx, p, x, y);
    }
    RTEN_LAUNCH_CHECK(ctx, "pad_b32");
    return RTEN_HIP_OK;
}
