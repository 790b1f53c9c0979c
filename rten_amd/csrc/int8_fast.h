// What the three units of the fast int8 path share (the overview is the header comment of int8_fast.hip):
//   int8_stage.hip       staging kernels, their launchers, and the entry points that only stage (prepack, staged quantizers, statistics blocks)
//   int8_fast.hip        igemm_i8_fast_kernel and the dispatch of its launch forms
//   int8_fast_entry.hip  the entry points that fill a FastArgs and dispatch it (GEMM, convolution, quantized output, quantize-on-load)
// Layouts: a staged operand is CHUNK-MAJOR signed bytes [Kp/16][rows][16 B], Kp = K rounded up to KT, followed (weights) by int32[rows] row sums at
// up256(rows * Kp); a staged convolution input is the padded channel-blocked image [N][Cp/16][Hp][Wp][16 B] that ConvGeom describes, or its PACKED form.
#pragma once
#include "internal.h"

namespace {
constexpr int KT = 64; // k bytes per tile (4 chunks of 16)
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int gemm_kp(int k) { return (k + KT - 1) / KT * KT; }
inline bool gemm_b_covered(int k, int n) { return k > 0 && n > 0 && k <= (1 << 18) && (long long)n * gemm_kp(k) < (1ll << 31); } // K bound: the kernel's chunk table lives in LDS

constexpr unsigned kSyncCtlWords = 16;    // exchange block: word 0 = departures, word 8 = time-out flag, then kSyncGranules 8-byte {min, max} granules
constexpr unsigned kSyncGranules = 2048;  // >= the workgroups the device holds at once (8 per compute unit x 256)
constexpr unsigned kSyncWords = kSyncCtlWords + 2 * kSyncGranules;

// The argument block of igemm_i8_fast_kernel (unnamed namespace, like the kernel that takes it by value: the other units pass it to the dispatcher by address)
struct FastArgs {
    const uint8_t *A;      // [M][Kp] signed rows
    const uint8_t *B;      // GEMM: [N][Kp] signed rows; conv: padded NHWC image
    const int *rsum;       // [M] sums of A rows
    const int *csum;       // [N] sums of B rows (GEMM) or NULL (conv: accumulated in-kernel when needed)
    void *C;
    const uint8_t *a_zp, *b_zp;
    const float *scale, *bias, *res;
    int M, N, Kp, Kreal;
    unsigned a_bytes, b_bytes;
    long long c_rs, c_ns;
    int Pn;
    int a_signed, b_signed, a_zp_len, b_zp_len, scale_len, relu, need_csum;
    int scale_per_row; // conv: scale[m] per output channel instead of scale[0] / scale[n]
    unsigned *stats;   // optional: min/max of the f32 outputs, accumulated for the DynamicQuantizeLinear that consumes them
    int tiles_m, tiles_n, n_fastest;
    // conv geometry (padded image)
    int conv, OW, sy, sx, Hp, Wp, Cp, KH, KW, dy, dx;
    // BQ kernels (DynamicQuantizeLinear fused into the B loader of a pointwise conv): the f32 activations, the min/max block their
    // producer left, the plane size, and where the quantizer's own outputs go
    const float *xf;
    const unsigned *in_stats;
    int HW, Cin;
    float *xs_out;
    uint8_t *xz_out;
    // QO kernels (the DynamicQuantizeLinear that CONSUMES this convolution's output runs in its epilogue, behind a grid-wide min / max):
    // the barrier block, the consumer's staged image and its geometry, the quantizer's own outputs
    unsigned *sync;
    unsigned *fault; // the context's sticky fault word (host-mapped): written only when a grid-wide wait gives up
    uint8_t *q_out;
    float *q_scale_out;
    uint8_t *q_zp_out;
    const float *q_mul_by;
    float *q_product;
    int q_cb, q_Hp, q_Wp, q_pt, q_pl, q_H, q_W, q_pad_mode;
    unsigned q_bytes;
    int debug_flags; // RTEN_HIP_DEBUG tuning switches seen by the kernel (bit 0: general zero-point algebra everywhere)
    // KS kernels (cross-workgroup K split): `ks` workgroups share one output tile, each sums its slice of the k-tiles, parks the raw int32 partial in `slab`
    // ([tile][part][wave][register quad][lane] x 16 B) and arrives on the tile's counter; the last arrival adds the others' partials to its own registers
    // (integer addition: any order gives the same bits) and runs the epilogue
    int ks;
    int *slab;
    unsigned *ks_counters;
    int no_store; // statistics-only launch (pass 1 of the recompute form of a quantized output): the epilogue runs, nothing is stored
    // exact division by the conv geometry's run-time divisors as multiply + shift (filled by launch_fast): the prologue's per-lane
    // pixel decode and the chunk table otherwise spend ~40 VALU instructions per division, on every resident wave at once
    RtenDiv d_pn, d_ow, d_cpc, d_kw, d_hw, d_qw, d_tile;
};

// RT: the single-row-term zero-point algebra of the convolution form (weight zero point 0 in the signed domain, one activation zero point)
inline bool single_row_term(const FastArgs &a) { return a.conv && !(a.debug_flags & 1) && a.a_zp == nullptr && a.a_signed && a.b_zp_len <= 1 && !a.need_csum; }
} // namespace

// `packed` (round 6): the few-channel form of stage_packed_chunks -- C <= 4 input channels and a kernel at least two columns wide.  The choice depends on C, KW
// and the group count ONLY: weights are prepacked from a descriptor that knows nothing else (ConvInteger::prepack), and every zero-point form stays exact -- the
// unused bytes of a chunk are 0 in the signed domain on BOTH operands, like the padded channels of the 16-channel-block form, so they add nothing to the product,
// the row sums or the column sums.  Cp / Wp / taps / Kp / img then describe the VIRTUAL convolution the kernel walks (16 channels, KW = nch, stride nch over
// OW * nch virtual columns); sx / kw / dx say so to the launch.
struct ConvGeom { int Cp, Hp, Wp, taps, Kreal, Kp, P; size_t img; bool ok; bool packed; int nch, cpc, sx, kw, dx; };

ConvGeom rten_i8_conv_geom(const rten_hip_conv2d_int8_desc *di);
// int8_stage.hip, launchers (the caller checks the launch): rows of a strided u8 / i8 matrix -> staged operand + row sums (k-contiguous rows or not);
// OIHW convolution weights -> staged operand of the geometry `g` + row sums; a u8 / i8 NCHW image -> the staged input of `g` (border: the effective pad mode)
void rten_i8_pack_rows(rten_hip_ctx *ctx, const void *src, long long row_stride, long long k_stride, int rows, int k, int Kp, unsigned flip, char *dst, char *sums);
void rten_i8_pack_conv_weights(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const ConvGeom &g, const void *w, void *dst, void *sums);
void rten_i8_stage_image(rten_hip_ctx *ctx, const rten_hip_conv2d_int8_desc *di, const ConvGeom &g, const void *x, const void *x_zp, void *staged);
// int8_fast.hip: `args` = the caller's FastArgs, complete but for the tile fields.  Picks the launch form from it (q_out + in_stats: recompute; q_out: exchange;
// xf: quantize-on-load; ks: may split K; else plain) and the tile from the context's rule, launches under the kernel's label and checks the launch.
// RTEN_HIP_ERR_UNSUPPORTED, nothing launched: an exchange grid that cannot be resident at once, or a recompute launch outside the single-row-term form.
int32_t rten_i8_dispatch_fast(rten_hip_ctx *ctx, void *args, double ops, double bytes);
