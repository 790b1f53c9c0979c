// Entry points of the fast int8 path: each stages what the caller has not staged (int8_stage.hip), fills a FastArgs and hands it to the dispatcher
// (int8_fast.hip).  The GEMM and convolution forms are called by int8.hip; the quantized-output and quantize-on-load forms are C ABI entry points.
#include "int8_fast.h"

namespace {

// The convolution half of a FastArgs for weights staged at `w` (row sums behind them): output shape and strides, K, operand A, the epilogue's inputs.  What
// differs between the callers -- B and its size, the geometry the kernel walks, the zero-point side -- they spell out themselves.
void fill_conv_args(FastArgs &g, const rten_hip_conv2d_int8_desc *di, const ConvGeom &cg, const void *w, const float *scale, const float *bias, const float *residual,
                    uint32_t flags, void *y) {
    const rten_hip_conv2d_desc *d = &di->conv;
    g.A = (const uint8_t *)w;
    g.rsum = (const int *)((const char *)w + up256((size_t)d->o * cg.Kp));
    g.C = y;
    g.scale = scale; g.bias = bias;
    g.res = (flags & RTEN_HIP_CONV_RESIDUAL) ? residual : nullptr;
    g.relu = (flags & RTEN_HIP_CONV_RELU) ? 1 : 0;
    g.M = d->o; g.N = d->n * cg.P; g.Kp = cg.Kp; g.Kreal = cg.Kreal;
    g.a_bytes = (unsigned)((size_t)d->o * cg.Kp);
    g.c_rs = cg.P; g.c_ns = (long long)d->o * cg.P; g.Pn = cg.P;
    g.a_signed = di->w_signed;
    g.scale_len = scale ? 1 : 0;
    g.scale_per_row = (scale && di->scale_len > 1) ? 1 : 0;
    g.conv = 1; g.OW = d->out_w; g.Cp = cg.Cp;
}

struct QOutArgs { // the consumer side of rten_hip_conv2d_int8_qout
    const rten_hip_conv2d_int8_desc *next;
    void *sync, *staged;
    float *scale;
    uint8_t *zp;
    const float *mul_by;
    float *product;
};

// The quantized-output fields (both forms): where the consumer's codes and the quantizer's own outputs go, and the consumer's staged geometry `ng`
void fill_qout_args(FastArgs &g, const QOutArgs &qo, const ConvGeom &ng, const rten_hip_conv2d_desc *d) {
    g.q_out = (uint8_t *)qo.staged;
    g.q_scale_out = qo.scale; g.q_zp_out = qo.zp; g.q_mul_by = qo.mul_by; g.q_product = qo.product;
    g.q_cb = ng.Cp / 16; g.q_Hp = ng.Hp; g.q_Wp = ng.Wp; g.q_pt = qo.next->conv.pads[0]; g.q_pl = qo.next->conv.pads[1];
    g.q_H = d->out_h; g.q_W = d->out_w; g.q_pad_mode = rten_effective_pad_mode(qo.next);
    g.q_bytes = (unsigned)ng.img;
}

int32_t i8_fast_conv_impl(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const void *x, const void *w, const void *x_zp, const void *w_zp,
                          const float *scale, const float *bias, const float *residual, uint32_t flags, void *y, void *stats, const QOutArgs *qo) {
    const rten_hip_conv2d_desc *d = &di->conv;
    const ConvGeom cg = rten_i8_conv_geom(di);
    if (!cg.ok)
        return (di->weights_packed || di->x_staged) ? rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "conv_int8: staged operands for an unsupported geometry")
                                                    : RTEN_HIP_ERR_UNSUPPORTED;
    const size_t wbytes = di->weights_packed ? 0 : up256((size_t)d->o * cg.Kp) + up256((size_t)d->o * 4);
    // cross-workgroup K split (KS kernels): a slab for up to kKsMax int32 partials of the (tile-padded) output, for the launches the dispatcher may split
    constexpr int kKsMax = 4;
    const long long n_cols = (long long)d->n * cg.P;
    const long long t64 = (long long)((d->o + 63) / 64) * ((n_cols + 63) / 64);
    static const bool ks_knob = getenv("RTEN_I8_KS") != nullptr && atoi(getenv("RTEN_I8_KS")) >= 2; // (no slab, no scratch growth, unless the measurement knob is set)
    const bool ks_candidate = ks_knob && !qo && scale && !(flags & RTEN_HIP_CONV_RESIDUAL) && cg.Kp >= 16 * 64 && t64 <= 3 * (long long)ctx->num_cus && ctx->split_counters;
    const size_t slab_bytes = ks_candidate ? (size_t)kKsMax * (size_t)((d->o + 127) / 128 * 128) * (size_t)((n_cols + 127) / 128 * 128) * 4 : 0;
    const size_t offA = 4096, offB = offA + wbytes, offS = offB + (di->x_staged ? 0 : up256(cg.img)), total = offS + slab_bytes;
    char *sc = (char *)rten_scratch(ctx, total);
    if (!sc) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "int8 staging allocation failed (or attempted during graph capture)");
    if (!di->weights_packed) rten_i8_pack_conv_weights(ctx, di, cg, w, sc + offA, sc + offA + up256((size_t)d->o * cg.Kp));
    if (!di->x_staged) rten_i8_stage_image(ctx, di, cg, x, x_zp, sc + offB);
    RTEN_LAUNCH_CHECK(ctx, "int8 staging launch");
    FastArgs g = {};
    fill_conv_args(g, di, cg, di->weights_packed ? w : sc + offA, scale, bias, residual, flags, y);
    g.B = di->x_staged ? (const uint8_t *)x : (const uint8_t *)(sc + offB);
    g.csum = nullptr;
    g.a_zp = di->w_zp_len ? (const uint8_t *)w_zp : nullptr;
    g.b_zp = (const uint8_t *)x_zp;
    g.b_bytes = (unsigned)cg.img;
    g.b_signed = di->x_signed;
    g.a_zp_len = di->w_zp_len; g.b_zp_len = x_zp ? 1 : 0;
    g.stats = scale ? (unsigned *)stats : nullptr;
    g.need_csum = (di->w_zp_len != 0 || !di->w_signed) ? 1 : 0; // weight zero point may be non-zero in the signed domain
    g.debug_flags = (ctx->debug & 0x200000) ? 1 : 0;
    g.sy = d->stride_h; g.sx = cg.sx; g.Hp = cg.Hp; g.Wp = cg.Wp;
    g.KH = d->kh; g.KW = cg.kw; g.dy = d->dil_h; g.dx = cg.dx; // (cg.sx / kw / dx: the virtual geometry of a few-channel packed image, else the convolution's own)
    if (slab_bytes) { g.ks = kKsMax; g.slab = (int *)(sc + offS); g.ks_counters = ctx->split_counters; }
    const double ops = 2.0 * d->o * (double)g.N * cg.Kreal, in_bytes = (double)d->o * cg.Kreal + (double)d->n * d->c * d->h * d->w;
    double out_bytes = 4.0 * d->o * g.N;
    if (qo && !qo->sync) {
        // Recompute form (no exchange block): launch 1 = this convolution, statistics only (nothing stored); launch 2 = the same convolution again, which
        // folds those statistics, quantizes in its epilogue and writes the consumer's staged image (+ the f32 tensor when `y` is wanted)
        if (!stats) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "conv2d_int8_qout (recompute form): a statistics block is required");
        // (this site used to test the predicate without `conv` and `b_zp_len <= 1`: g.conv is 1 and g.b_zp_len is 0 or 1 by the lines above, so the full one gives the same value)
        if (!single_row_term(g) || g.res) return RTEN_HIP_ERR_UNSUPPORTED; // (built for the single-row-term form without a residual: the caller runs the two operators)
        FastArgs g1 = g;
        g1.no_store = 1;
        const int32_t rc1 = rten_i8_dispatch_fast(ctx, &g1, ops, in_bytes);
        if (rc1 != RTEN_HIP_OK) return rc1;
        const ConvGeom ng = rten_i8_conv_geom(qo->next);
        g.in_stats = (const unsigned *)stats;
        g.stats = nullptr;
        fill_qout_args(g, *qo, ng, d);
        g.ks = 0; g.slab = nullptr;
        return rten_i8_dispatch_fast(ctx, &g, ops, in_bytes + (y ? out_bytes : 0.0) + (double)ng.img);
    }
    if (qo) {
        const ConvGeom ng = rten_i8_conv_geom(qo->next);
        g.sync = (unsigned *)qo->sync;
        g.fault = ctx->fault_dev;
        fill_qout_args(g, *qo, ng, d);
        out_bytes = (y ? out_bytes : 0.0) + (double)ng.img;
    }
    // algorithmic bytes: i8 weights + u8 activations (once) + f32 output (+ f32 residual when the epilogue adds one); quantized-output form:
    // the consumer's staged u8 image instead of (or, when y is wanted too, besides) the f32 output
    return rten_i8_dispatch_fast(ctx, &g, ops, in_bytes + out_bytes + (g.res ? 4.0 * d->o * g.N : 0.0));
}

__global__ void grid_sync_reset_kernel(unsigned *sync, int count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; // one thread per word
    if (i >= (long long)count * kSyncWords) return;
    const unsigned w = (unsigned)(i % kSyncWords);
    sync[i] = (w >= kSyncCtlWords && ((w - kSyncCtlWords) & 1u) == 0u) ? 0xffffffffu : 0u; // granule = {lo = 0xffffffff, hi = 0}
}

} // namespace

// Entry points used by int8.hip: return RTEN_HIP_ERR_UNSUPPORTED when the fast path does not cover the call
// (the caller then falls back to the generic kernel).
int32_t rten_i8_fast_gemm(rten_hip_ctx *ctx, const rten_hip_gemm_int8_desc *d, const void *a, const void *b, const void *a_zp,
                          const void *b_zp, const float *scale, void *c) {
    const int Kp = gemm_kp(d->k);
    if (d->k <= 0 || (long long)d->m * Kp >= (1ll << 31) || !gemm_b_covered(d->k, d->n) || (long long)d->m * d->ldc >= (1ll << 29))
        return RTEN_HIP_ERR_UNSUPPORTED;
    // per call: the activation side (A) is staged; B too unless the caller prepacked it at load (MatMulInteger weights)
    const size_t b_img = up256((size_t)d->n * Kp);
    const size_t offA = 4096, offRs = offA + up256((size_t)d->m * Kp), offB = offRs + up256((size_t)d->m * 4),
                 offCs = offB + (d->b_prepacked ? 0 : b_img), total = offCs + (d->b_prepacked ? 0 : up256((size_t)d->n * 4));
    char *sc = (char *)rten_scratch(ctx, total);
    if (!sc) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "int8 staging allocation failed (or attempted during graph capture)");
    rten_i8_pack_rows(ctx, a, d->a_rs, d->a_cs, d->m, d->k, Kp, d->a_signed ? 0u : 0x80u, sc + offA, sc + offRs);
    if (!d->b_prepacked) rten_i8_pack_rows(ctx, b, d->b_cs, d->b_rs, d->n, d->k, Kp, d->b_signed ? 0u : 0x80u, sc + offB, sc + offCs);
    RTEN_LAUNCH_CHECK(ctx, "i8_pack_rows_kernel launch");
    FastArgs g = {};
    g.A = (const uint8_t *)(sc + offA);
    g.B = d->b_prepacked ? (const uint8_t *)b : (const uint8_t *)(sc + offB);
    g.rsum = (const int *)(sc + offRs);
    g.csum = d->b_prepacked ? (const int *)((const char *)b + b_img) : (const int *)(sc + offCs);
    g.C = c;
    g.a_zp = d->a_zp_len ? (const uint8_t *)a_zp : nullptr;
    g.b_zp = d->b_zp_len ? (const uint8_t *)b_zp : nullptr;
    g.scale = d->scale_len ? scale : nullptr;
    g.M = d->m; g.N = d->n; g.Kp = Kp; g.Kreal = d->k;
    g.a_bytes = (unsigned)((size_t)d->m * Kp); g.b_bytes = (unsigned)((size_t)d->n * Kp);
    g.c_rs = d->ldc; g.c_ns = 0; g.Pn = d->n;
    g.a_signed = d->a_signed; g.b_signed = d->b_signed;
    g.a_zp_len = d->a_zp_len; g.b_zp_len = d->b_zp_len; g.scale_len = d->scale_len;
    return rten_i8_dispatch_fast(ctx, &g, 2.0 * d->m * (double)d->n * d->k, (double)d->m * d->k + (double)d->k * d->n + 4.0 * d->m * d->n);
}

int32_t rten_i8_fast_conv(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const void *x, const void *w, const void *x_zp,
                          const void *w_zp, const float *scale, const float *bias, const float *residual, uint32_t flags, void *y, void *stats) {
    return i8_fast_conv_impl(ctx, di, x, w, x_zp, w_zp, scale, bias, residual, flags, y, stats, nullptr);
}

// ConvIntegerToFloat [+ bias] [+ residual] [+ Relu] AND the DynamicQuantizeLinear of the one convolution that consumes its output, in ONE
// launch (igemm_i8_fast_kernel, QO): see rten_hip.h.  RTEN_HIP_ERR_UNSUPPORTED when the geometry is not covered or the launch's
// workgroups cannot all be resident at once -- run rten_hip_conv2d_int8_stats + rten_hip_dynamic_quantize_linear_staged_stats then.
RTEN_EXPORT size_t rten_hip_grid_sync_bytes(void) { return kSyncWords * sizeof(unsigned); }

RTEN_EXPORT int32_t rten_hip_conv2d_int8_qout(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const void *x, const void *w, const void *x_zp,
                                              const void *w_zp, const float *scale, const float *bias, const float *residual, uint32_t flags, float *y,
                                              void *stats, void *sync, const rten_hip_conv2d_int8_desc *next, void *next_staged, float *next_scale,
                                              uint8_t *next_zero_point, const float *mul_by, float *product) {
    RTEN_CHECK_CTX(ctx);
    if (!di || !x || !w || !scale || !stats || !next || !next_staged || !next_scale || !next_zero_point || (mul_by && !product))
        return RTEN_HIP_ERR_INVALID_VALUE; // (sync == NULL: the recompute form -- two launches, no grid-wide exchange, no residency requirement)
    const rten_hip_conv2d_desc *d = &di->conv, *nd = &next->conv;
    if (di->scale_len != 0 && di->scale_len != 1 && di->scale_len != d->o)
        return rten_set_error(ctx, RTEN_HIP_ERR_INCOMPATIBLE_SHAPES, "conv_int8: scale must be a scalar or have one value per output channel");
    if (di->w_zp_len != 0 && di->w_zp_len != 1 && di->w_zp_len != d->o) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "Zero point has incorrect size");
    if (nd->n != d->n || nd->c != d->o || nd->h != d->out_h || nd->w != d->out_w)
        return rten_set_error(ctx, RTEN_HIP_ERR_INCOMPATIBLE_SHAPES, "conv2d_int8_qout: the consumer's input is not this convolution's output");
    const ConvGeom cg = rten_i8_conv_geom(di), ng = rten_i8_conv_geom(next);
    if (!cg.ok || !ng.ok || ng.packed || next->x_signed || !di->weights_packed || !di->x_staged || d->o % 16 != 0)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "conv2d_int8_qout: staged operands, O % 16 == 0 and a consumer covered by the staged kernel only");
    if (d->n == 0 || d->out_h == 0 || d->out_w == 0) return RTEN_HIP_OK;
    const QOutArgs qo = {next, sync, next_staged, next_scale, next_zero_point, mul_by, product};
    return i8_fast_conv_impl(ctx, di, x, w, x_zp, w_zp, scale, bias, residual, flags, y, stats, &qo);
}

// Initialises `count` consecutive exchange blocks (once, when they are allocated; every launch leaves its block in this state).
RTEN_EXPORT int32_t rten_hip_grid_sync_reset(rten_hip_ctx *ctx, void *sync, int32_t count) {
    RTEN_CHECK_CTX(ctx);
    if (!sync || count < 1) return RTEN_HIP_ERR_INVALID_VALUE;
    // the reset ends with a stream synchronise (the sticky fault is cleared after what is in flight has drained): inside a capture that would
    // invalidate the capture instead of resetting anything -- refused, not attempted
    if (ctx->capturing) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "grid_sync_reset: not while a graph capture is active on this context");
    const long long n = (long long)count * kSyncWords;
    hipLaunchKernelGGL(grid_sync_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (unsigned *)sync, count);
    RTEN_LAUNCH_CHECK(ctx, "grid_sync_reset_kernel launch");
    if (ctx->fault_host) { // the caller starts over: the context's sticky fault goes with the blocks' flags (after what is in flight has drained)
        RTEN_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        *ctx->fault_host = 0u;
    }
    return RTEN_HIP_OK;
}

// Time-out flags of `count` consecutive barrier blocks (non-zero: a quantized-output launch gave up waiting for its grid and its results are void).
RTEN_EXPORT int32_t rten_hip_grid_sync_timeouts(rten_hip_ctx *ctx, const void *sync, int32_t count, int32_t *timeouts) {
    RTEN_CHECK_CTX(ctx);
    if (!sync || count < 1 || !timeouts) return RTEN_HIP_ERR_INVALID_VALUE;
    std::vector<unsigned> host((size_t)count * kSyncWords);
    RTEN_HIP_TRY(ctx, hipMemcpyAsync(host.data(), sync, host.size() * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    RTEN_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int n = 0;
    for (int i = 0; i < count; i++) n += host[(size_t)i * kSyncWords + 8] != 0;
    *timeouts = n;
    return RTEN_HIP_OK;
}

// DynamicQuantizeLinear -> ConvInteger -> Cast -> Mul(x_scale, w_scale) [-> Add(bias)] [-> Add(residual)] [-> Relu] of a dynamically
// quantized graph in ONE launch, for pointwise (1x1, stride 1, no padding, groups 1) convolutions whose input statistics were
// accumulated by the producing kernel (rten_hip_conv2d_int8_stats / this function): the quantizer runs inside the B loader of the
// integer GEMM (igemm_i8_fast_kernel, BQ).  `w` must be prepacked (rten_hip_conv2d_int8_prepack), `w_scale` is the scalar or
// per-output-channel weight scale (di->scale_len), `x_scale_out` / `x_zero_point_out` receive DynamicQuantizeLinear's own outputs
// (optional).  RTEN_HIP_ERR_UNSUPPORTED for any other geometry: run the staged sequence instead.
RTEN_EXPORT int32_t rten_hip_conv2d_int8_dql(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const float *x, const void *in_stats, const void *w,
                                             const float *w_scale, const float *bias, const float *residual, uint32_t flags, float *y, void *out_stats,
                                             float *x_scale_out, uint8_t *x_zero_point_out) {
    RTEN_CHECK_CTX(ctx);
    if (!di || !x || !in_stats || !w || !w_scale || !y) return RTEN_HIP_ERR_INVALID_VALUE;
    const rten_hip_conv2d_desc *d = &di->conv;
    const ConvGeom cg = rten_i8_conv_geom(di);
    const bool pointwise = d->kh == 1 && d->kw == 1 && d->stride_h == 1 && d->stride_w == 1 && d->groups == 1 && d->pads[0] == 0 && d->pads[1] == 0 &&
                           d->pads[2] == 0 && d->pads[3] == 0;
    if (!cg.ok || !pointwise || !di->weights_packed || di->x_signed || di->w_zp_len != 0 || d->c % 64 != 0 ||
        (long long)d->n * d->c * d->h * d->w * 4 >= (1ll << 31))
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "conv2d_int8_dql: pointwise stride-1 unpadded convolutions with prepacked weights and C % 64 == 0 only");
    if (di->scale_len != 0 && di->scale_len != 1 && di->scale_len != d->o)
        return rten_set_error(ctx, RTEN_HIP_ERR_INCOMPATIBLE_SHAPES, "conv_int8: scale must be a scalar or have one value per output channel");
    if (d->n == 0 || d->out_h == 0 || d->out_w == 0) return RTEN_HIP_OK;
    FastArgs g = {};
    fill_conv_args(g, di, cg, w, w_scale, bias, residual, flags, y);
    g.xf = x; g.in_stats = (const unsigned *)in_stats; g.HW = d->h * d->w; g.Cin = d->c;
    g.xs_out = x_scale_out; g.xz_out = x_zero_point_out;
    g.b_bytes = (unsigned)((size_t)d->n * d->c * d->h * d->w * 4);
    g.b_signed = 0;
    g.a_zp_len = 0; g.b_zp_len = 1;
    g.stats = (unsigned *)out_stats;
    g.need_csum = di->w_signed ? 0 : 1;
    g.sy = 1; g.sx = 1; g.Hp = d->h; g.Wp = d->w; g.KH = 1; g.KW = 1; g.dy = 1; g.dx = 1; // the unpadded f32 tensor itself, one tap
    // algorithmic bytes: i8 weights + f32 activations (read once) + f32 output (+ f32 residual)
    return rten_i8_dispatch_fast(ctx, &g, 2.0 * d->o * (double)g.N * cg.Kreal,
                                 (double)d->o * cg.Kreal + 4.0 * d->n * d->c * d->h * d->w + 4.0 * d->o * g.N + (g.res ? 4.0 * d->o * g.N : 0.0));
}
