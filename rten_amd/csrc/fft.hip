// DFT and STFT (src/ops/fft.rs:22-373) on one transform core: a Stockham autosort FFT on complex f32 that stays in LDS from load to store.
//
// Plan (fft_plan, host): a length n is a product of passes -- radix 4 as often as it divides, then one 2, then 3s and 5s (specialised butterflies in
// registers), then every other prime factor <= 31 as a generic pass.  A length with a prime factor above 31 is ONE direct pass of radix n.
// Pass of radix r at stride s (the product of the radices before it), m = n / (s r), for butterfly b = q + s p (q < s, p < m):
//     a_j = src[b + s m j]                                   j < r     (consecutive butterflies read consecutive words)
//     dst[q + s (r p + k)] = (sum_j a_j W_r^(j k)) * W_n^(p s k)   k < r
// which is the decimation-in-frequency Stockham step: after the last pass the data stands in natural order, no bit reversal.  Every twiddle is an
// INTEGER index into one table w[t] = exp(-/+ 2 pi i t / n), t < n: W_r^(jk) = w[(jk mod r) n / r], W_n^(psk) = w[p s k] (p s k < n, no reduction
// needed).  No angle is ever formed in f32.  The table is written by fft_twiddle_kernel into the context's auxiliary scratch at every call, each entry
// from float64 sincospi(2k / n) rounded once.
//   * specialised passes (2, 3, 4, 5): a thread owns one butterfly per iteration, operands in registers; 2 and 4 use adds and exact +-i rotations only.
//   * generic and direct passes: a thread owns one OUTPUT (b, k) per iteration and sums its r products in order j = 0 .. r-1, reading a_j from LDS; the
//     index (j k) mod r is carried by adding k and subtracting r on wrap, exact for r up to 8191.
// A workgroup of 256 threads carries lanes_per_wg = max(1, 256 r_max / n) whole lanes (at most 8192 points in all), so short transforms keep every thread
// busy; the last workgroup may be partial.  Two ping-pong buffers; a logical index i lives at i + (i >> 5): one float2 of padding per 64-dword bank row,
// which spreads the power-of-two output strides s r of a pass over the banks (docs/KERNELS.md 4.16).
// Loaders (FFT_DFT: truncate / zero-fill; FFT_IRFFT: conjugate-half rebuild; FFT_STFT: frames read straight from the signal, times the window) and the
// storer (first out_len bins, 1 or 2 components, the inverse's scale) wrap the same core.  Loads and stores are scalar floats: operands need 4-byte
// alignment only.  Every output element is written exactly once; nothing else is written; no atomics, no read-back.
#include "internal.h"

namespace {

constexpr int FFT_THREADS = 256;
constexpr int FFT_MAX_PASSES = 16;
enum { FFT_DFT = 0, FFT_IRFFT = 1, FFT_STFT = 2 };

struct FftPass {
    int32_t r, s, bpl; // radix, stride (product of earlier radices), butterflies per lane = n / r
    RtenDiv div_s, div_bpl, div_r;
};

struct FftArgs {
    int32_t n, npass, lanes_per_wg, mode;
    int32_t buf_elems;             // float2 elements of one ping-pong buffer (padding included)
    int32_t comp, n_copy, conj_end; // input components; points copied from the input lane; IRFFT: mirror k in [1, conj_end)
    int32_t out_len, out_comp, apply_scale;
    float scale;
    int64_t lanes, n_in;           // n_in: points of an input lane (DFT) / samples of a batch row (STFT)
    int64_t n_frames, frame_step;
    RtenDiv div_n, div_out;
    FftPass pass[FFT_MAX_PASSES];
};

template <bool PAD> __device__ __forceinline__ int fft_at(int i) { return PAD ? i + (i >> 5) : i; }
__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

__global__ __launch_bounds__(FFT_THREADS) void fft_twiddle_kernel(int n, int inverse, float2 *__restrict__ w) {
    const int k = blockIdx.x * FFT_THREADS + threadIdx.x;
    if (k >= n) return;
    double s, c;
    sincospi(2.0 * (double)k / (double)n, &s, &c);
    const float sf = (float)s;
    w[k] = make_float2((float)c, inverse ? sf : 0.0f - sf);
}

// one specialised pass of compile-time radix R over `items` butterflies of the workgroup's lanes
template <int R, bool PAD>
__device__ __forceinline__ void fft_pass_fixed(const FftPass &ps, int n, int items, bool inverse, const float2 *__restrict__ tw, const float2 *src, float2 *dst) {
    float2 wr[R]; // W_R^t, t < R (3 and 5 only)
    if constexpr (R == 3 || R == 5) {
#pragma unroll
        for (int t = 0; t < R; t++) wr[t] = tw[t * (n / R)];
    }
    for (int it = threadIdx.x; it < items; it += FFT_THREADS) {
        const int l = rten_div(it, ps.div_bpl), b = it - l * ps.bpl;
        const int p = rten_div(b, ps.div_s), q = b - p * ps.s;
        const int base = l * n;
        float2 a[R], o[R];
#pragma unroll
        for (int j = 0; j < R; j++) a[j] = src[fft_at<PAD>(base + b + ps.bpl * j)];
        if constexpr (R == 2) {
            o[0] = cadd(a[0], a[1]);
            o[1] = csub(a[0], a[1]);
        } else if constexpr (R == 4) {
            const float2 t0 = cadd(a[0], a[2]), t1 = csub(a[0], a[2]), t2 = cadd(a[1], a[3]), t3 = csub(a[1], a[3]);
            const float2 rot = inverse ? make_float2(-t3.y, t3.x) : make_float2(t3.y, -t3.x); // (+i or -i) * t3, exact
            o[0] = cadd(t0, t2);
            o[2] = csub(t0, t2);
            o[1] = cadd(t1, rot);
            o[3] = csub(t1, rot);
        } else {
#pragma unroll
            for (int k = 0; k < R; k++) {
                float2 acc = a[0];
#pragma unroll
                for (int j = 1; j < R; j++) acc = cadd(acc, k == 0 ? a[j] : cmul(a[j], wr[(j * k) % R]));
                o[k] = acc;
            }
        }
        const int ob = base + q + ps.s * R * p, t1 = p * ps.s;
        dst[fft_at<PAD>(ob)] = o[0];
#pragma unroll
        for (int k = 1; k < R; k++) dst[fft_at<PAD>(ob + ps.s * k)] = p ? cmul(o[k], tw[t1 * k]) : o[k];
    }
}

// a generic pass (odd prime r <= 31) or the direct pass (r == n): one output per thread and iteration
template <bool PAD>
__device__ __forceinline__ void fft_pass_generic(const FftPass &ps, int n, int nl, const RtenDiv &div_n, const float2 *__restrict__ tw, const float2 *src, float2 *dst) {
    const int r = ps.r, wstride = n / r, items = nl * n;
    for (int it = threadIdx.x; it < items; it += FFT_THREADS) {
        const int l = rten_div(it, div_n), o = it - l * n;
        const int b = rten_div(o, ps.div_r), k = o - b * r;
        const int p = rten_div(b, ps.div_s), q = b - p * ps.s;
        const int base = l * n;
        float2 acc = src[fft_at<PAD>(base + b)];
        int t = k; // (j k) mod r at j = 1
        for (int j = 1; j < r; j++) {
            acc = cadd(acc, cmul(src[fft_at<PAD>(base + b + ps.bpl * j)], tw[t * wstride]));
            t += k;
            if (t >= r) t -= r;
        }
        if (p && k) acc = cmul(acc, tw[p * ps.s * k]);
        dst[fft_at<PAD>(base + q + ps.s * (r * p + k))] = acc;
    }
}

template <bool PAD>
__global__ __launch_bounds__(FFT_THREADS) void fft_kernel(const FftArgs a, const float2 *__restrict__ tw, const float *__restrict__ x, const float *__restrict__ win,
                                                          float *__restrict__ y) {
    extern __shared__ float2 fft_lds[];
    __shared__ int64_t lane_in[FFT_THREADS]; // where each of the workgroup's lanes starts in x, in floats
    const int n = a.n;
    const int64_t lane0 = (int64_t)blockIdx.x * a.lanes_per_wg;
    const int nl = (int)(a.lanes - lane0 < a.lanes_per_wg ? a.lanes - lane0 : a.lanes_per_wg);
    if ((int)threadIdx.x < nl) {
        const int64_t g = lane0 + threadIdx.x;
        if (a.mode == FFT_STFT) {
            const int64_t b = g / a.n_frames, f = g - b * a.n_frames;
            lane_in[threadIdx.x] = (b * a.n_in + f * a.frame_step) * a.comp;
        } else {
            lane_in[threadIdx.x] = g * a.n_in * a.comp;
        }
    }
    __syncthreads();
    float2 *src = fft_lds, *dst = fft_lds + a.buf_elems;
    const int total = nl * n;
    for (int i = threadIdx.x; i < total; i += FFT_THREADS) {
        const int l = rten_div(i, a.div_n), k = i - l * n;
        const float *lane = x + lane_in[l];
        float2 v = make_float2(0.f, 0.f);
        if (a.mode == FFT_STFT) {
            v.x = lane[(int64_t)k * a.comp];
            if (a.comp == 2) v.y = lane[(int64_t)k * 2 + 1];
            if (win) { const float w = win[k]; v.x = w * v.x; v.y = a.comp == 2 ? w * v.y : 0.f; }
        } else {
            const int mk = n - k; // IRFFT: the bin whose conjugate stands at k
            if (a.mode == FFT_IRFFT && k >= 1 && mk >= 1 && mk < a.conj_end) {
                v.x = lane[(int64_t)mk * 2];
                v.y = -lane[(int64_t)mk * 2 + 1];
            } else if (k < a.n_copy) {
                v.x = lane[(int64_t)k * a.comp];
                if (a.comp == 2) v.y = lane[(int64_t)k * 2 + 1];
            }
        }
        src[fft_at<PAD>(i)] = v;
    }
    __syncthreads();
    const bool inverse = a.apply_scale != 0;
    for (int ps = 0; ps < a.npass; ps++) {
        const FftPass &P = a.pass[ps];
        const int items = nl * P.bpl;
        switch (P.r) {
        case 4: fft_pass_fixed<4, PAD>(P, n, items, inverse, tw, src, dst); break;
        case 2: fft_pass_fixed<2, PAD>(P, n, items, inverse, tw, src, dst); break;
        case 3: fft_pass_fixed<3, PAD>(P, n, items, inverse, tw, src, dst); break;
        case 5: fft_pass_fixed<5, PAD>(P, n, items, inverse, tw, src, dst); break;
        default: fft_pass_generic<PAD>(P, n, nl, a.div_n, tw, src, dst); break;
        }
        __syncthreads();
        float2 *t = src; src = dst; dst = t;
    }
    const int total_out = nl * a.out_len;
    for (int i = threadIdx.x; i < total_out; i += FFT_THREADS) {
        const int l = rten_div(i, a.div_out), k = i - l * a.out_len;
        float2 v = src[fft_at<PAD>(l * n + k)];
        if (a.apply_scale) { v.x = v.x * a.scale; v.y = v.y * a.scale; }
        float *o = y + ((lane0 + l) * a.out_len + k) * a.out_comp;
        o[0] = v.x;
        if (a.out_comp == 2) o[1] = v.y;
    }
}

// the pass list of a length: count, or a negative code
int fft_plan(int64_t n, int32_t *radices, int32_t capacity) {
    if (n < 1 || !radices || capacity < 0) return -RTEN_HIP_ERR_INVALID_VALUE;
    if (n > RTEN_HIP_FFT_MAX) return -RTEN_HIP_ERR_UNSUPPORTED;
    int32_t tmp[FFT_MAX_PASSES];
    int cnt = 0;
    int64_t rest = n;
    while (rest % 4 == 0) { tmp[cnt++] = 4; rest /= 4; }
    if (rest % 2 == 0) { tmp[cnt++] = 2; rest /= 2; }
    for (int p = 3; p <= RTEN_HIP_FFT_GENERIC_RADIX_MAX; p += 2)
        while (rest % p == 0) { tmp[cnt++] = p; rest /= p; } // (a composite p never divides: its prime factors are gone by then)
    if (rest != 1) { cnt = 0; tmp[cnt++] = (int32_t)n; }       // a prime factor above the generic limit: one direct pass
    if (cnt > capacity) return -RTEN_HIP_ERR_INVALID_VALUE;
    for (int i = 0; i < cnt; i++) radices[i] = tmp[i];
    return cnt;
}

int32_t fft_launch(rten_hip_ctx *ctx, FftArgs &a, const char *what, const float *x, const float *win, float *y, double bytes) {
    int32_t radices[FFT_MAX_PASSES];
    const int n = a.n;
    const int cnt = fft_plan(n, radices, FFT_MAX_PASSES);
    if (cnt < 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "%s: no plan for length %d", what, n);
    a.npass = cnt;
    int r_max = 1, s = 1;
    for (int i = 0; i < cnt; i++) {
        FftPass &P = a.pass[i];
        P.r = radices[i];
        P.s = s;
        P.bpl = n / P.r;
        P.div_s = rten_make_div(1 << 14, P.s);
        P.div_bpl = rten_make_div(1 << 14, P.bpl);
        P.div_r = rten_make_div(1 << 14, P.r);
        s *= P.r;
        if (P.r > r_max) r_max = P.r;
    }
    int lpw = (int)((int64_t)FFT_THREADS * r_max / n);
    if (lpw > RTEN_HIP_FFT_MAX / n) lpw = RTEN_HIP_FFT_MAX / n; // the LDS cap: at most 8192 points per buffer
    if (lpw > FFT_THREADS) lpw = FFT_THREADS;
    if (lpw < 1) lpw = 1;
    a.lanes_per_wg = lpw;
    a.div_n = rten_make_div(1 << 14, n);
    a.div_out = rten_make_div(1 << 14, a.out_len);
    const bool pad = !(ctx->debug & (1 << 20)); // ablation bit: unpadded buffers, to read the bank-conflict counter against
    const int points = lpw * n;
    a.buf_elems = pad ? points + (points >> 5) + 1 : points;
    const size_t lds = (size_t)a.buf_elems * 2 * sizeof(float2);
    float2 *tw = (float2 *)rten_aux_scratch(ctx, (size_t)n * sizeof(float2));
    if (!tw) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "%s: the twiddle table's scratch cannot be allocated (inside a capture: run once eagerly first)", what);
    const int64_t wgs = ceil_div64(a.lanes, lpw);
    {
        ProfScope ps(ctx, "fft_twiddle", 0.0, 8.0 * n);
        hipLaunchKernelGGL(fft_twiddle_kernel, dim3((unsigned)ceil_div64(n, FFT_THREADS)), dim3(FFT_THREADS), 0, ctx->stream, n, a.apply_scale, tw);
        RTEN_LAUNCH_CHECK(ctx, "fft_twiddle");
    }
    ProfScope ps(ctx, what, 5.0 * (double)a.lanes * n * (cnt ? cnt : 1) * 2, bytes);
    if (pad) {
        if (lds > 64 * 1024) RTEN_HIP_TRY(ctx, hipFuncSetAttribute((const void *)fft_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(fft_kernel<true>, dim3((unsigned)wgs), dim3(FFT_THREADS), lds, ctx->stream, a, (const float2 *)tw, x, win, y);
    } else {
        if (lds > 64 * 1024) RTEN_HIP_TRY(ctx, hipFuncSetAttribute((const void *)fft_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(fft_kernel<false>, dim3((unsigned)wgs), dim3(FFT_THREADS), lds, ctx->stream, a, (const float2 *)tw, x, win, y);
    }
    RTEN_LAUNCH_CHECK(ctx, what);
    return RTEN_HIP_OK;
}

constexpr int64_t kFftLim = (int64_t)1 << 31;

} // namespace

RTEN_EXPORT int32_t rten_hip_fft_plan(int64_t n, int32_t *radices, int32_t capacity) { return fft_plan(n, radices, capacity); }

RTEN_EXPORT int32_t rten_hip_dft_f32(rten_hip_ctx *ctx, int64_t lanes, int64_t n_in, int64_t n_fft, int32_t in_components, int32_t inverse, int32_t onesided,
                                     const float *x, float *y) {
    RTEN_CHECK_CTX(ctx);
    if (lanes < 0 || n_in < 0 || n_fft < 0 || lanes >= kFftLim || n_in >= kFftLim) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "dft: bad dimension");
    if (in_components != 1 && in_components != 2) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "Last dimension of DFT input must have size 1 or 2");
    const bool irfft = inverse && onesided, rfft = onesided && !inverse;
    if (irfft && in_components != 2) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "Inverse one-sided DFT (IRFFT) requires complex input");
    if (rfft && in_components == 2) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "DFT cannot be one-sided if input is complex");
    if (n_fft > RTEN_HIP_FFT_MAX)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "DFT of length %lld exceeds the limit of %d points (RTEN_HIP_FFT_MAX)", (long long)n_fft, RTEN_HIP_FFT_MAX);
    if (lanes == 0) return RTEN_HIP_OK;
    if (n_fft == 0) {
        if (!rfft) return RTEN_HIP_OK;
        if (!y) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "dft: null output");
        RTEN_HIP_TRY(ctx, hipMemsetAsync(y, 0, (size_t)lanes * 2 * sizeof(float), ctx->stream)); // one zero bin per lane (fft.rs:263-265)
        return RTEN_HIP_OK;
    }
    const int64_t n_copy = n_in < n_fft ? n_in : n_fft;
    if (!y || (!x && n_copy > 0)) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "dft: null input or output");
    FftArgs a = {};
    a.n = (int32_t)n_fft;
    a.mode = irfft ? FFT_IRFFT : FFT_DFT;
    a.comp = in_components;
    a.n_copy = (int32_t)n_copy;
    a.conj_end = (int32_t)(n_fft % 2 == 0 ? (n_copy > 0 ? n_copy - 1 : 0) : n_copy);
    a.out_len = (int32_t)(rfft ? n_fft / 2 + 1 : n_fft);
    a.out_comp = irfft ? 1 : 2;
    a.apply_scale = inverse ? 1 : 0;
    a.scale = inverse ? 1.0f / (float)n_fft : 1.0f;
    a.lanes = lanes;
    a.n_in = n_in;
    a.n_frames = 1;
    a.frame_step = 0;
    return fft_launch(ctx, a, irfft ? "irfft_f32" : (inverse ? "idft_f32" : (rfft ? "rfft_f32" : "dft_f32")), x, nullptr, y,
                      4.0 * lanes * ((double)n_copy * in_components + (double)a.out_len * a.out_comp));
}

RTEN_EXPORT int32_t rten_hip_stft_f32(rten_hip_ctx *ctx, int64_t batch, int64_t signal_len, int32_t components, int64_t frame_step, int64_t n_fft, int32_t onesided,
                                      const float *window_or_null, const float *signal, float *y) {
    RTEN_CHECK_CTX(ctx);
    if (batch < 0 || signal_len < 0 || batch >= kFftLim || signal_len >= ((int64_t)1 << 40)) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "stft: bad dimension");
    if (n_fft != 0 && (n_fft < 1 || n_fft > signal_len)) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "frame_length must be in range [1, signal_length]");
    if (frame_step <= 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "frame_step must be > 0");
    if (components != 1 && components != 2) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "Last dimension of signal must have size 1 or 2");
    if (components == 2 && onesided) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "FFT cannot be one-sided if input is complex");
    if (batch == 0 || n_fft == 0) return RTEN_HIP_OK;
    if (n_fft > RTEN_HIP_FFT_MAX)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "STFT frame of length %lld exceeds the limit of %d points (RTEN_HIP_FFT_MAX)", (long long)n_fft, RTEN_HIP_FFT_MAX);
    if (!signal || !y) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "stft: null signal or output");
    const int64_t n_frames = (signal_len - n_fft) / frame_step + 1;
    if ((double)batch * (double)n_frames >= (double)kFftLim) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "stft: bad dimension");
    FftArgs a = {};
    a.n = (int32_t)n_fft;
    a.mode = FFT_STFT;
    a.comp = components;
    a.n_copy = (int32_t)n_fft;
    a.out_len = (int32_t)(onesided ? n_fft / 2 + 1 : n_fft);
    a.out_comp = 2;
    a.apply_scale = 0;
    a.scale = 1.0f;
    a.lanes = batch * n_frames;
    a.n_in = signal_len;
    a.n_frames = n_frames;
    a.frame_step = frame_step;
    return fft_launch(ctx, a, "stft_f32", signal, window_or_null, y, 4.0 * batch * ((double)signal_len * components + (double)n_frames * a.out_len * 2));
}
