// MFMA f32 tiled GEMM / implicit-GEMM convolution for gfx950 (MI355X).
//
// Replaces: GemmExecutor::gemm / gemm_uninit / batched_gemm_uninit (rten-gemm/src/lib.rs:255-372,
// gemm_impl :794-1093), the f32 micro-kernel (kernels/simd_generic.rs:285-414), the virtual
// im2col packing (rten-gemm/src/im2col.rs:56-212, src/ops/conv/im2col.rs:11-128) and conv_impl /
// conv_2d_pointwise (src/ops/conv.rs:33-87,124-365).
//
// This file is the host side: the launch plans (launch_cfg: split-K, tail, persistent and thin-tile decisions; pick_cfg; dispatch), the
// variant table, the tuning setters, the GEMM and convolution entry points, weight prepacking and the im2col table cache.  The kernels
// live one family per translation unit, each behind one rten_launch_gemm_f32_<family> function (internal.h): gemm_f32_reg.hip
// (register-staged), _dma.hip (LDS-DMA and the split-K fixup), _dma16.hip (16x16x4 MFMAs), _pers.hip / _lean.hip (persistent), _ws.hip
// (wave-specialised), _thin.hip (thin-tile tail), _smallm.hip (small-M streaming), _wave.hip, _patch.hip, _stem.hip, _pair.hip; what they
// share (argument block, prologue helpers, fold / epilogue, split-K finish) is gemm_f32_common.h.
//
// One kernel template covers GEMM and convolution:
//     C[m, n] = epilogue( sum_k A[m, k] * B[k, n] )
//   * conv:  m = output channel, k = (c, ky, kx), n = (image, oy, ox) flattened over the WHOLE batch, so
//            late ResNet stages (7x7 / 14x14 maps) still produce thousands of columns per launch.
//            B is never materialised: the im2col gather is fused into the global->LDS tile load.
//            1x1/stride-1 convs skip the gather and read the NCHW tensor as a "two-level" matrix
//            (column n -> image n / P, pixel n % P).
//   * C is written straight into NCHW (row m, two-level column n), with bias / residual Add / Relu /
//     Gelu fused into the epilogue.
//
// MI355X mapping
//   * v_mfma_f32_32x32x2_f32 (exact f32, 64 FLOP/clk/SIMD == the f32 peak, 157 TF).  256 threads = 4
//     waves per workgroup, each wave owns TM x TN accumulator tiles of 32x32.
//   * A and B tiles are staged through LDS k-major ([BK][BM+pad], [BK][BN+pad]) so the MFMA operand
//     fetch (lane -> row k0 + lane/32, column lane%32) is a conflict-free ds_read_b32; tiles are double
//     buffered, the next tile's global loads are issued before the current tile's MFMAs (one barrier
//     per k-tile).
//   * The f32 matrix pipe is slow (64 cycles per MFMA), so the kernel is bound by how few OTHER
//     instructions each wave issues per MFMA.  All global loads are raw buffer loads
//     (buffer_load_dword/dwordx4 ... offen) whose per-lane byte offsets are loop invariant; the k-tile
//     advance rides in the scalar soffset operand, and out-of-tile / out-of-image / k-tail lanes point
//     at an out-of-range offset so the hardware returns 0 -- no exec-mask branches, no 64-bit address
//     arithmetic and no selects in the K loop.  The im2col (c, ky, kx) decomposition comes from a small
//     per-geometry lookup table read with scalar loads (the k row of a wave is uniform).
//   * Workgroup ids are remapped so that each XCD (private L2) owns a contiguous range of tiles that
//     share the same B panel.
//
// Numerics: accumulation order is the reference's, exactly: k-ordered FMA chain per depth block of
// kc = 256 starting from 0, blocks combined with separate adds, bias added after the first block
// (rten-gemm/src/lib.rs:630-633,1008-1013,1221-1255; simd_generic.rs:378-414).  MFMA f32 is a
// k-ordered fmaf chain bit for bit, so outputs are bit-identical to the oracle for M > 1.
#include "gemm_f32_common.h"

namespace {

// im2col lookup table: entry k -> {c*HW + ky*dy*W + kx*dx, (ky*dy) | (kx*dx) << 16}; rows >= K get an
// offset pair that fails every bounds test.  taps != 0 (B_IM2COL_TAPS): the second word is 31 - (ky*KW + kx), the
// left shift that moves the tap's padding bit of the per-lane mask to bit 31; rows >= K use shift 0 (bit 31 is
// always set in the masks).  Built once per conv geometry and cached in the context.
__global__ void im2col_lut_kernel(i32x2 *lut, int K, int Kpad, int KHW, int KW, int HW, int W, int dy, int dx, int taps) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Kpad) return;
    if (k >= K) { lut[k] = taps ? i32x2{0, 0} : i32x2{0, 0xffff}; return; } // dy = 65535 > any padded height
    const int c = k / KHW, rem = k - c * KHW, ky = rem / KW, kx = rem - ky * KW;
    lut[k] = i32x2{c * HW + ky * dy * W + kx * dx, taps ? 31 - rem : (ky * dy) | ((kx * dx) << 16)};
}
} // namespace

// =====================================================================================================
// Host side: variant selection and the C-ABI entry points
// =====================================================================================================
namespace {

struct TileCfg { int bm, bn; float penalty; };
constexpr TileCfg kCfgs[4] = {{128, 128, 1.00f}, {128, 64, 1.04f}, {64, 128, 1.04f}, {64, 64, 1.12f}};

// The GEMM variants (rten_hip_set_gemm_variant_override; the ids are part of the tuning interface): tile shape (index into kCfgs), pipeline
// and wave flavour of each.  Non-conv operand layouts always use the register-staged kernel; a launch a variant's kernels do not cover runs
// as variant 3.  Any other id (-1 = automatic) is kAutoVariant: the cost model picks the tile shape.
struct Variant { int cfg, pipeline, wave_flavour; };
constexpr Variant kAutoVariant = {-1, 1, 0};
constexpr Variant kVariants[] = {
    {0, 1, 0}, {1, 1, 0}, {2, 1, 0}, {3, 1, 0}, //  0..3  the four tile shapes on the three-stage LDS-DMA pipeline (conv paths)
    {0, 0, 0}, {1, 0, 0}, {2, 0, 0}, {3, 0, 0}, //  4..7  ... on the register-staged pipeline
    {0, 2, 0}, {1, 2, 0}, {2, 2, 0}, {3, 2, 0}, //  8..11 ... LDS-DMA with wave specialisation (4 MFMA waves + 4 loader waves)
    {0, 3, 0}, {1, 3, 0}, {2, 3, 0}, {3, 3, 0}, // 12..15 ... LDS-DMA with four LDS stages
    {0, 4, 0}, {1, 4, 0}, {2, 4, 0}, {3, 4, 0}, // 16..19 ... LDS-DMA, fragments-first MFMA issue
    {0, 5, 0}, {1, 5, 0}, {2, 5, 0}, {3, 5, 0}, // 20..23 ... LDS-DMA on 16x16x4 MFMAs
    {3, 6, 0},                                  // 24 one wave per 64x64 tile (gemm_f32_wave.hip), k-tile 16 x 2 LDS stages
    {3, 6, 1},                                  // 25 ... 8 x 4
    {3, 6, 2},                                  // 26 ... 16 x 3
    {3, 7, 0},                                  // 27 64x64 LDS-DMA with TWO stages
    {3, 6, 4},                                  // 28 one wave per 32x32 tile (barrier-free form of the 64x64 / 4-wave granularity; dense B), 16 x 2
    {3, 6, 5},                                  // 29 ... 16 x 3
    {3, 8, 0},                                  // 30 3x3 / stride 1 / padding 1 convolutions with B staged as image patches (gemm_f32_patch.hip)
    {3, 1, 0},                                  // 31 small-M weight streaming (rten_hip_gemm_f32 with one batch and M <= 64: gemm_f32_smallm.hip; also what -1 picks there)
    {3, 1, 0},                                  // 32 3-channel 7x7 stride-2 convolutions with prepacked weights as a direct implicit GEMM (gemm_f32_stem.hip; also what -1 picks there)
};
constexpr int kNumVariants = (int)(sizeof kVariants / sizeof kVariants[0]);
constexpr const Variant &variant_row(int v) { return v >= 0 && v < kNumVariants ? kVariants[v] : kAutoVariant; }

// The table against the range rule it replaced (the setter's ternary chain and pick_cfg's range tests, as they were).
constexpr bool variants_as_ever() {
    if (kNumVariants != 33) return false;
    for (int v = 0; v < 33; v++) {
        const int flavour = (v >= 24 && v < 27) ? v - 24 : (v >= 28 && v < 30) ? v - 24 : 0;
        const int pipeline = v == 30 ? 8 : v == 27 ? 7 : (v >= 24 && v < 30) ? 6 : (v >= 20 && v < 24) ? 5 : (v >= 16 && v < 20) ? 4 : (v >= 12 && v < 16) ? 3 : (v >= 8 && v < 12) ? 2 : (v >= 4 && v < 8) ? 0 : 1;
        const int cfg = v >= 24 ? 3 : v & 3;
        if (kVariants[v].cfg != cfg || kVariants[v].pipeline != pipeline || kVariants[v].wave_flavour != flavour) return false;
    }
    return true;
}
static_assert(variants_as_ever(), "a GEMM variant id changed its tile shape, pipeline or wave flavour");

// Dynamic LDS (bytes the kernel never touches) that makes exactly `n` workgroups of `static_bytes` fit the 160 KB of a compute unit: the
// dispatcher places workgroups wherever a slot is free, so only LDS pins the count.  `largest`: the most each of the n can hold (rounded
// down to 1 KB under a 256-byte allowance) -- the persistent plans; otherwise the least that keeps workgroup n + 1 out (rounded up to 256
// bytes over a 1 KB allowance) -- the occupancy cap.
inline int lds_pad_for_workgroups(int n, int static_bytes, bool largest) {
    constexpr int kCuLds = 160 * 1024;
    const int dyn = largest ? (kCuLds / n - static_bytes - 256) & ~1023 : (kCuLds / (n + 1) + 1024 - static_bytes + 255) & ~255;
    return dyn > 0 ? dyn : 0;
}

// Occupancy cap of the LDS-DMA kernels (order bits 4-6 = workgroups per compute unit, 0 = whatever fits).  Why a cap: with one 32x32
// accumulator block per wave every MFMA of a wave depends on its previous one, and three or more such waves on a SIMD share the matrix pipe
// badly (tools/debug/f32_trace.py: 64x64 tiles at 3-4 workgroups per CU keep it 67 % busy inside the k-loop; tools/probes/kloop.hip row A:
// 150 TF/s at two waves per SIMD, 114 at three).
inline size_t occupancy_pad(const rten_hip_ctx *ctx, int static_bytes) {
    static const int env_cap = getenv("RTEN_HIP_OCC_CAP") ? atoi(getenv("RTEN_HIP_OCC_CAP")) : 0; // tuning only
    const int cap = env_cap > 0 ? env_cap : (ctx->tile_order >> 4) & 7;
    if (cap < 2) return 0; // (a cap of 1 needs more than 64 KB per workgroup: not offered)
    return (size_t)lds_pad_for_workgroups(cap, static_bytes, false);
}

// One launch plan for every pipeline: whole tiles [0, t1) by the folding kernel (MODE 0/1), split tiles [t1, T) by
// the split-K producer (MODE 2) followed by the ordered fixup.  Only depth-block boundaries are legal K cuts.
// Which kernel families exist for a (tile shape, A layout, B layout) is decided here; the families' launchers
// (rten_launch_gemm_f32_<family>, one translation unit each) refuse a combination they have no kernel for.
int32_t launch_cfg(rten_hip_ctx *ctx, GemmArgs &a, int Z, int BM, int BN, int AL, int BL) {
    a.tiles_m = (a.M + BM - 1) / BM;
    a.tiles_n = (a.N + BN - 1) / BN;
    const double flops = 2.0 * a.M * (double)a.N * a.K * Z;
    const double bytes = 4.0 * Z * ((double)a.M * a.K + (double)a.K * a.N + (double)a.M * a.N);
    const bool multi = a.K > 256;
    const bool kDma = (AL == A_M4 || AL == A_K4) && (BL == B_N4 || BL == B_IM2COL || BL == B_IM2COL_TAPS);
    const bool t64 = BM == 64 && BN == 64;
    int pipe = kDma ? ctx->pipeline : 0;
    if (AL == A_K4 && pipe == 2) pipe = 1; // the wave-specialised kernel only takes k-major A
    if (pipe == 6 && !(AL == A_M4 && t64)) pipe = 1; // the wave-tile kernels: prepacked weights, 64x64 tiles
    if (pipe == 6 && ctx->wave_flavour >= 4 && BL != B_N4) pipe = 1; // 32x32 wave tiles: dense B only
    if (pipe == 7 && !t64) pipe = 1;                                 // the two-stage ring exists for 64x64 tiles
    const bool want_patch = pipe == 8 && AL == A_M4 && t64 && (BL == B_IM2COL || BL == B_IM2COL_TAPS) && ctx->split_mode < 4; // (split modes 4..6 are kernels of their own)
    if (pipe == 8 && !want_patch) pipe = 1;                          // the patch kernels: prepacked weights, 64x64 tiles, im2col B; anything else (and a launch they refuse) runs variant 3
    if (BL == B_IM2COL_TAPS && pipe == 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "internal: tap-mask im2col needs an LDS-DMA pipeline");

    const int nblk = (a.K + 255) / 256;
    const int T = a.tiles_m * a.tiles_n;
    int ntail = 0, t1 = T, S = 1;
    a.split_s = 1;
    a.order = ctx->tile_order & 3;
    const bool relaxed_split = (ctx->tile_order & 8) != 0 && (pipe == 1 || pipe == 3 || pipe == 4 || pipe == 7); // igemm_f32_dma_kernel only
    int split_mode = ctx->split_mode, split_req = ctx->split_s;
    if (pipe == 6 && ctx->wave_flavour >= 4) split_mode = 0; // (no split-K form: whole tiles only)
    if (split_mode == 3) { // auto: too few tiles to fill the chip -> cut every tile so that ~num_cus workgroups exist
        const long long wgs = (long long)T * Z;
        split_mode = (multi && wgs * 2 <= ctx->num_cus) ? 2 : 0;
        split_req = (int)(ctx->num_cus / (wgs > 0 ? wgs : 1));
    }
    if (multi && pipe != 2 && pipe != 5 && split_mode > 0 && split_mode < 4 && split_req > 1) { // (the wave-specialised and 16x16x4 kernels have no split-K form)
        const int s_req = split_req < nblk ? split_req : nblk;
        const int G = (nblk + s_req - 1) / s_req;
        S = (nblk + G - 1) / G;
        t1 = split_mode == 2 ? 0 : (T / ctx->num_cus) * ctx->num_cus;
        if (S > 1 && t1 < T) {
            ntail = T - t1;
            a.split_t1 = t1; a.split_s = S; a.split_g = G; a.split_slots = relaxed_split ? S : nblk; a.split_ntail = ntail;
            if (relaxed_split) a.order |= 8;
            const size_t need = 4096 + (size_t)Z * ntail * nblk * BM * BN * sizeof(float);
            char *sc = (char *)rten_scratch(ctx, need);
            if (!sc) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "split-K slab allocation failed (or attempted during graph capture)");
            a.slab = (float *)(sc + 4096);
            // the last-arriving producer folds the tile in the same launch (split_finish); RTEN_HIP_DEBUG bit 0x80000 keeps the fixup kernel
            a.split_counters = (!(ctx->debug & 0x80000) && (long long)Z * ntail <= rten_hip_ctx::kSplitCounters) ? ctx->split_counters : nullptr;
        } else {
            t1 = T;
        }
    }

    const int dma_static = 3 * BK * (BM + BN) * 4; // LDS of the three-stage ring
    // One launch of whole tiles (mode 0 / 1) or split-K producers (mode 2) on the plan's pipeline.
    auto launch = [&](int mode, unsigned gx, double fl, double by) -> int32_t {
        const unsigned gz = (unsigned)Z;
        if (pipe == 6) { // one wave per tile (gemm_f32_wave.hip)
            char kname[96];
            snprintf(kname, sizeof kname, "igemm_f32_wave_kernel<%d,%d,%d>", BL, mode, ctx->wave_flavour);
            ProfScope ps(ctx, kname, fl, by);
            return rten_launch_gemm_f32_wave(ctx, &a, gx, gz, BL, mode, ctx->wave_flavour);
        }
        if (pipe == 8) { // image patches instead of per-element gathers (gemm_f32_patch.hip): 3x3 / stride 1 / padding 1 only
            char kname[96];
            snprintf(kname, sizeof kname, "igemm_f32_patch_kernel<%d>", mode);
            ProfScope ps(ctx, kname, fl, by);
            const int32_t rc = rten_launch_gemm_f32_patch(ctx, &a, gx, gz, mode);
            if (rc != RTEN_HIP_ERR_UNSUPPORTED) return rc;
            pipe = 1; // a geometry the patch family does not cover: the three-stage LDS-DMA kernel
        }
        if (pipe == 2 && mode == 1 && a.act > RTEN_HIP_ACT_GELU) pipe = 1; // the multi-block warp-specialised kernel's epilogue stops at Gelu: the three-stage kernel
        switch (pipe) {
        case 2: return rten_launch_gemm_f32_ws(ctx, &a, gx, gz, BM, BN, BL, mode, fl, by);
        case 1: return rten_launch_gemm_f32_dma(ctx, &a, gx, gz, BM, BN, AL, BL, mode, 3, 0, occupancy_pad(ctx, dma_static), fl, by);
        case 4: return rten_launch_gemm_f32_dma(ctx, &a, gx, gz, BM, BN, AL, BL, mode, 3, 1, 0, fl, by); // fragments first, MFMAs back to back (see MFK)
        case 5: return rten_launch_gemm_f32_dma16(ctx, &a, gx, gz, BM, BN, AL, BL, mode, fl, by); // 16x16x4 MFMAs: four independent accumulators per 32x32 of a wave's share
        case 7: return rten_launch_gemm_f32_dma(ctx, &a, gx, gz, BM, BN, AL, BL, mode, 2, 0, 0, fl, by); // TWO LDS stages (16 KB per workgroup): up to 7 workgroups per compute unit instead of 6 -- the other workgroups are the prefetch depth
        case 3: return rten_launch_gemm_f32_dma(ctx, &a, gx, gz, BM, BN, AL, BL, mode, 4, 0, 0, fl, by); // four LDS stages: three k-tiles in flight behind the one being multiplied
        default: return rten_launch_gemm_f32_reg(ctx, &a, gx, gz, BM, BN, AL, BL, mode, fl, by);
        }
    };

    // Lean persistent plan (split mode 6, groups = resident workgroups per compute unit): igemm_f32_lean_kernel, 64x64 tiles, for
    // the convolution form (prepacked weights, one group, alpha = 1 / beta = 0) with K a multiple of 32; other calls ignore it.
    if (AL == A_M4 && (BL == B_N4 || BL == B_IM2COL_TAPS) && t64 && ctx->split_mode == 6 && Z == 1 && a.batch_inner <= 1 && a.alpha == 1.f &&
        a.beta == 0.f && a.bias_kind != RTEN_HIP_BIAS_PER_COL && a.K % LBK == 0 && a.K >= LBK && T > 1 && a.a_bs == (long long)a.K * a.a_cs) {
        // groups = workgroups per compute unit + 10 * (LDS stages - 3): 1..3 (three stages), 11, 12 (four), 21, 22 (five)
        const int nst = 3 + (ctx->split_s / 10 > 2 ? 2 : ctx->split_s / 10);
        int per_cu = ctx->split_s % 10;
        const int lean_static = nst * LBK * 128 * 4;
        const int max_cu = 160 * 1024 / lean_static;
        per_cu = per_cu < 1 ? 1 : (per_cu > max_cu ? max_cu : per_cu);
        long long G = (long long)ctx->num_cus * per_cu;
        if (G > T) G = T;
        a.split_slots = ctx->num_cus; // (unused by this kernel's arithmetic: carries num_cus for the de-phasing delay)
        a.debug = (ctx->tile_order & 2) ? 0x100 : 0; // order bit 1 = de-phase co-resident workgroups (tuning knob)
        return rten_launch_gemm_f32_lean(ctx, &a, (unsigned)G, BL, nst, lds_pad_for_workgroups(per_cu, lean_static, true), flops, bytes);
    }

    // Persistent plan (split mode 5, groups = resident workgroups per compute unit): one launch of num_cus x groups workgroups
    // that walk the tile list with the tile DMA running across tile boundaries (igemm_f32_pers_kernel).
    if (kDma && ctx->split_mode == 5 && (pipe == 1 || pipe == 4 || pipe == 5) && T > 1) {
        const int per_cu = ctx->split_s < 1 ? 1 : (ctx->split_s > 4 ? 4 : ctx->split_s);
        long long G = (long long)ctx->num_cus * per_cu;
        if (G > T) G = T;
        return rten_launch_gemm_f32_pers(ctx, &a, (unsigned)G, (unsigned)Z, BM, BN, AL, BL, pipe == 5 ? 2 : pipe == 4 ? 1 : 0,
                                         lds_pad_for_workgroups(per_cu, dma_static, true), flops, bytes);
    }

    // Thin-tile tail plan (split mode 4; convolution form alpha = 1, beta = 0, one group): the whole rounds of num_cus tiles go
    // to this tile shape over columns [0, n_big), the remaining columns to the 16x64 kernel on 16x16x4 MFMAs, whose quarter-size
    // per-SIMD blocks finish the tail in a quarter of a round (see igemm_f32_thin_kernel).  Same bits as any other plan.
    if (kDma && AL == A_M4 && ctx->split_mode == 4 && Z == 1 && a.batch_inner <= 1 && a.alpha == 1.f && a.beta == 0.f && a.bias_kind != RTEN_HIP_BIAS_PER_COL) {
        const long long rounds = T / ctx->num_cus;
        const long long big_cols = rounds * ctx->num_cus / a.tiles_m; // column tiles that fit into the whole rounds
        const long long big_tiles = big_cols * a.tiles_m;
        if (rounds >= 1 && big_cols >= 1 && big_cols * BN < a.N) {
            const int n_big = (int)(big_cols * BN);
            GemmArgs th = a;
            th.n_lo = n_big;
            th.tiles_m = (a.M + 15) / 16;
            const int thin_tiles_n = (a.N - n_big + 63) / 64;
            a.N = n_big; // the whole tiles stop at n_big; output addressing is unchanged
            a.tiles_n = n_big / BN;
            const double frac_big = (double)n_big / th.N;
            const int32_t rc = launch(multi ? 1 : 0, (unsigned)big_tiles, flops * frac_big, bytes * frac_big);
            if (rc) return rc;
            return rten_launch_gemm_f32_thin(ctx, &th, (unsigned)(th.tiles_m * thin_tiles_n), BL, multi, flops * (1.0 - frac_big), bytes * (1.0 - frac_big));
        }
    }

    const bool mixed = kDma && BM * BN < 128 * 128 && pipe == 1 && ntail > 0 && t1 > 0;
    if (mixed) { // whole tiles and the tail's split-K producers in ONE launch (co-resident), then the fixup
        const int32_t rc = rten_launch_gemm_f32_dma(ctx, &a, (unsigned)(t1 + ntail * S), (unsigned)Z, BM, BN, AL, BL, 3, 3, 0, occupancy_pad(ctx, dma_static), flops, bytes);
        if (rc) return rc;
    } else if (t1 > 0) {
        const int32_t rc = launch(multi ? 1 : 0, (unsigned)t1, flops * t1 / T, bytes * t1 / T);
        if (rc) return rc;
    }
    if (ntail > 0) {
        if (!mixed) {
            const int32_t rc = launch(2, (unsigned)(ntail * S), flops * ntail / T, bytes * ntail / T);
            if (rc) return rc;
        }
        if (!a.split_counters) return rten_launch_gemm_f32_fixup(ctx, &a, (unsigned)ntail * 4u, (unsigned)Z, BM, BN, 8.0 * Z * ntail * nblk * BM * BN);
    }
    return RTEN_HIP_OK;
}

int pick_cfg(rten_hip_ctx *ctx, int M, long long N, int Z) {
    const int fixed = variant_row(ctx->gemm_variant_override).cfg;
    if (fixed >= 0) return fixed;
    int best = 3;
    double best_cost = 1e300;
    for (int c = 0; c < 4; c++) {
        const TileCfg &t = kCfgs[c];
        const long long tiles = (long long)((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn) * Z;
        const long long rounds = (tiles + ctx->num_cus - 1) / ctx->num_cus;
        const double cost = (double)rounds * t.bm * t.bn * t.penalty;
        if (cost < best_cost) { best_cost = cost; best = c; }
    }
    return best;
}

// al / bl: the operand layouts the caller found; the pairs no kernel loads with 16-byte accesses fall back to the scalar loaders.
int32_t dispatch(rten_hip_ctx *ctx, GemmArgs &a, int Z, int al, int bl) {
    const TileCfg &t = kCfgs[pick_cfg(ctx, a.M, a.N, Z)];
    const bool vec = (al == A_M4 && (bl == B_N4 || bl == B_IM2COL || bl == B_IM2COL_TAPS)) || (al == A_K4 && (bl == B_N4 || bl == B_K4));
    if (!vec) { al = A_SCALAR; bl = bl == B_IM2COL ? B_IM2COL : B_SCALAR; }
    return launch_cfg(ctx, a, Z, t.bm, t.bn, al, bl);
}

// Largest byte offset (exclusive) an operand slice with the given extents/strides can touch.
long long extent_bytes(long long rows, long long rs, long long cols, long long cs) {
    if (rows <= 0 || cols <= 0) return 4;
    return ((rows - 1) * rs + (cols - 1) * cs + 1) * 4;
}

constexpr long long kMaxBufBytes = 0x7fffffffll; // buffer offsets are 32-bit; the OOB marker is 2^31

} // namespace

RTEN_EXPORT int32_t rten_hip_num_gemm_variants(void) { return kNumVariants; }

RTEN_EXPORT int32_t rten_hip_set_gemm_variant_override(rten_hip_ctx *ctx, int32_t variant) {
    RTEN_CHECK_CTX(ctx);
    ctx->gemm_variant_override = variant;
    ctx->wave_flavour = variant_row(variant).wave_flavour;
    ctx->pipeline = variant_row(variant).pipeline;
    return RTEN_HIP_OK;
}

// Exact split-K plan: mode 0 = off, 1 = split only the tiles past the last full round of num_cus workgroups (tail
// balancing), 2 = split every tile, 3 = automatic (default: split every tile when fewer than num_cus/2 workgroups
// would exist); `groups` = K groups per split tile (modes 1, 2).  Mode 4 is not a K split: whole rounds of tiles plus a tail of
// thin 16x64 tiles on 16x16x4 MFMAs (convolutions; other calls run their plain plan).
RTEN_EXPORT int32_t rten_hip_set_gemm_split(rten_hip_ctx *ctx, int32_t mode, int32_t groups) {
    RTEN_CHECK_CTX(ctx);
    if (mode < 0 || mode > 6 || groups < 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "set_gemm_split: bad mode/groups");
    ctx->split_mode = mode;
    ctx->split_s = groups;
    return RTEN_HIP_OK;
}

// Workgroup -> tile order (tuning knob, sticky): bit 0 = tiles walk n fastest instead of m fastest; bit 1 = split-K
// workgroups walk tiles fastest and K groups slowest (each XCD's L2 then holds one K slice of both operands).
RTEN_EXPORT int32_t rten_hip_set_gemm_order(rten_hip_ctx *ctx, int32_t order) {
    RTEN_CHECK_CTX(ctx);
#ifdef RTEN_ABLATION // bit 3 = relaxed split-K (one partial per K group: NOT the reference's order, NOT bit-exact): measurement builds only
    constexpr int allowed = 0x7b;
#else
    constexpr int allowed = 0x73;
#endif
    if (order < 0 || (order & ~allowed)) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "set_gemm_order: bits 0-1 (tile walk) and 4-6 (workgroups per compute unit) only (bit 3, the relaxed split-K, exists in -DRTEN_ABLATION measurement builds)");
    ctx->tile_order = order;
    return RTEN_HIP_OK;
}

namespace {
int32_t gemm_f32_entry(rten_hip_ctx *ctx, const rten_hip_gemm_desc *d, const float *a, const float *b, const float *bias, float *c, bool allow_gemv,
                       const RtenAct *act = nullptr);
}

RTEN_EXPORT int32_t rten_hip_gemm_f32(rten_hip_ctx *ctx, const rten_hip_gemm_desc *d, const float *a, const float *b,
                                      const float *bias, float *c) {
    RTEN_CHECK_CTX(ctx);
    return gemm_f32_entry(ctx, d, a, b, bias, c, ctx->gemv_order != 0);
}

RTEN_EXPORT int32_t rten_hip_gemm_f32_act(rten_hip_ctx *ctx, const rten_hip_gemm_desc *d, const float *a, const float *b,
                                          const float *bias, int32_t act_kind, float act_alpha, float act_beta, float *c) {
    RTEN_CHECK_CTX(ctx);
    if (d && d->act != RTEN_HIP_ACT_NONE) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "gemm_act: desc.act must be NONE");
    if (!rten_act_valid(act_kind)) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "gemm_act: unknown activation kind");
    const RtenAct act = {act_kind, act_alpha, act_beta};
    return gemm_f32_entry(ctx, d, a, b, bias, c, ctx->gemv_order != 0, &act);
}

int32_t rten_gemm_f32_blocked(rten_hip_ctx *ctx, const rten_hip_gemm_desc *d, const float *a, const float *b, const float *bias, float *c) {
    RTEN_CHECK_CTX(ctx);
    return gemm_f32_entry(ctx, d, a, b, bias, c, false);
}

RTEN_EXPORT int32_t rten_hip_set_gemv_order(rten_hip_ctx *ctx, int32_t on, int32_t reference_threads) {
    RTEN_CHECK_CTX(ctx);
    if (reference_threads < 0) return RTEN_HIP_ERR_INVALID_VALUE;
    ctx->gemv_order = on ? 1 : 0;
    ctx->gemv_threads = reference_threads;
    return RTEN_HIP_OK;
}

namespace {
int32_t gemm_f32_entry(rten_hip_ctx *ctx, const rten_hip_gemm_desc *d, const float *a, const float *b, const float *bias, float *c, bool allow_gemv,
                       const RtenAct *act) {
    if (!d) return RTEN_HIP_ERR_INVALID_VALUE;
    if (d->m < 0 || d->n < 0 || d->k < 0 || d->batch < 0)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "gemm: negative dimension");
    if (d->bias_kind != RTEN_HIP_BIAS_NONE && !bias)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "gemm: bias_kind set but bias is NULL");
    if (d->m == 0 || d->n == 0 || d->batch == 0) return RTEN_HIP_OK; // rten-gemm/src/lib.rs:835-839
    if (!c || (d->k > 0 && (!a || !b))) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "gemm: NULL operand");
    if (d->ldc < d->n) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "gemm: ldc < n");
    if (d->a_rs < 0 || d->a_cs < 0 || d->b_rs < 0 || d->b_cs < 0)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "gemm: negative strides are not supported");
    // one row, B not prepacked: the reference takes its gemv kernels, whose accumulation order is not the blocked one (lib.rs:876-891)
    if (allow_gemv && d->m == 1 && d->k > 0) return rten_gemv_f32(ctx, d, a, b, bias, act, c);

    GemmArgs g = {};
    g.A = a ? a : c; g.B = b ? b : c; g.C = c; g.bias = bias; g.res = nullptr;
    g.M = d->m; g.N = d->n; g.K = d->k;
    g.a_rs = d->a_rs; g.a_cs = d->a_cs; g.a_bs = d->a_bs;
    g.b_rs = d->b_rs; g.b_cs = d->b_cs; g.b_ns = 0; g.b_bs = d->b_bs;
    g.c_rs = d->ldc; g.c_ns = 0; g.c_bs = d->c_bs;
    g.bias_bs = 0;
    g.batch_inner = d->batch_inner; g.a_bsi = d->a_bsi; g.b_bsi = d->b_bsi; g.c_bsi = d->c_bsi;
    g.Pn = d->n;
    g.alpha = d->alpha; g.beta = d->beta;
    g.bias_kind = d->bias_kind; g.act = d->act;
    if (act) { g.act = act->kind; g.act_a = act->alpha; g.act_b = act->beta; }
    g.a_dir_m = (d->a_rs == 1 && d->a_cs != 1) ? 1 : 0;
    g.b_dir_n = (d->b_cs == 1 || d->b_rs != 1) ? 1 : 0;
    const long long ab = extent_bytes(d->m, d->a_rs, d->k, d->a_cs), bb = extent_bytes(d->k, d->b_rs, d->n, d->b_cs);
    if (ab > kMaxBufBytes || bb > kMaxBufBytes || extent_bytes(d->m, d->ldc, d->n, 1) > kMaxBufBytes)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "gemm: operand slices above 2 GiB are not supported");
    g.a_bytes = (unsigned)ab; g.b_bytes = (unsigned)bb;

    // few rows: stream B through every compute unit instead of a handful of 64-row tiles (variant 31; the automatic choice; RTEN_HIP_DEBUG bit 0x40000 = off)
    if ((ctx->gemm_variant_override == 31 || (ctx->gemm_variant_override < 0 && !(ctx->debug & 0x40000))) && d->m <= 64 && d->batch == 1 && d->k > 0) {
        const int32_t rc = rten_launch_gemm_f32_smallm(ctx, &g, d, a, b);
        if (rc != RTEN_HIP_ERR_UNSUPPORTED) return rc;
    }

    int al = A_SCALAR, bl = B_SCALAR;
    if (d->k > 0) {
        const bool a4 = d->a_bs % 4 == 0 && d->a_bsi % 4 == 0 && aligned16(a), b4 = d->b_bs % 4 == 0 && d->b_bsi % 4 == 0 && aligned16(b);
        if (d->a_rs == 1 && d->a_cs % 4 == 0 && d->m % 4 == 0 && a4) al = A_M4;
        else if (d->a_cs == 1 && d->a_rs % 4 == 0 && d->k % 4 == 0 && a4) al = A_K4;
        if (d->b_cs == 1 && d->b_rs % 4 == 0 && d->n % 4 == 0 && b4) bl = B_N4;
        else if (d->b_rs == 1 && d->b_cs % 4 == 0 && d->k % 4 == 0 && b4) bl = B_K4;
        const bool have = (al == A_M4 && bl == B_N4) || (al == A_K4 && bl == B_N4) || (al == A_K4 && bl == B_K4);
        if (!have) { al = A_SCALAR; bl = B_SCALAR; }
    }
    return dispatch(ctx, g, d->batch, al, bl);
}
} // namespace

// ---- conv weight staging: W[g][m][k] (OIHW) -> packed[g][k][Og4], zero padded (Og4 = round_up(O/g, 4))
namespace {
__global__ void conv_prepack_f32_kernel(const float *__restrict__ w, float *__restrict__ packed, int groups, int Og,
                                        int K, int Og4) {
    const long long total = (long long)groups * K * Og4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(i % Og4);
        const long long r = i / Og4;
        const int k = (int)(r % K);
        const int g = (int)(r / K);
        packed[i] = m < Og ? w[((long long)g * Og + m) * K + k] : 0.f;
    }
}

int32_t check_conv_desc(rten_hip_ctx *ctx, const rten_hip_conv2d_desc *d) {
    if (!d) return RTEN_HIP_ERR_INVALID_VALUE;
    if (d->groups <= 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "Group count must be > 0");
    if (d->c % d->groups != 0)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "Input channel count not divisible by groups");
    if (d->o % d->groups != 0)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "Output channel count not divisible by groups");
    if (d->n < 0 || d->c <= 0 || d->h <= 0 || d->w <= 0 || d->o <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride_h <= 0 ||
        d->stride_w <= 0 || d->dil_h <= 0 || d->dil_w <= 0 || d->out_h < 0 || d->out_w < 0)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "conv: invalid geometry");
    const long long in_elems = (long long)d->n * d->c * d->h * d->w;
    const long long out_elems = (long long)d->n * d->o * d->out_h * d->out_w;
    if (in_elems * 4 > kMaxBufBytes || out_elems * 4 > kMaxBufBytes)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "conv: tensors above 2 GiB are not supported");
    if ((long long)d->kh * d->dil_h >= 0x7fff || (long long)d->kw * d->dil_w >= 0x7fff || d->h >= 0x7fff || d->w >= 0x7fff)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "conv: spatial extent above 32766 is not supported");
    return RTEN_HIP_OK;
}

// im2col LUT cache (per context): one table per (Cg, kh, kw, dil, H, W)
const i32x2 *get_im2col_lut(rten_hip_ctx *ctx, int Cg, int kh, int kw, int dy, int dx, int H, int W, int taps) {
    char key[96];
    snprintf(key, sizeof key, "%d.%d.%d.%d.%d.%d.%d.%d", Cg, kh, kw, dy, dx, H, W, taps);
    auto it = ctx->luts.find(key);
    if (it != ctx->luts.end()) return (const i32x2 *)it->second;
    if (ctx->capturing) return nullptr; // allocation is not capturable: warm up eagerly first
    const int K = Cg * kh * kw;
    const int Kpad = ((K + BK - 1) / BK + MAX_NSTAGE + 2) * BK; // tile / LUT look-ahead runs up to NSTAGE tiles past the end
    void *dptr = nullptr;
    if (hipMalloc(&dptr, (size_t)Kpad * sizeof(i32x2)) != hipSuccess) return nullptr;
    hipLaunchKernelGGL(im2col_lut_kernel, dim3((Kpad + 255) / 256), dim3(256), 0, ctx->stream, (i32x2 *)dptr, K, Kpad, kh * kw,
                       kw, H * W, W, dy, dx, taps);
    ctx->luts[key] = dptr;
    return (const i32x2 *)dptr;
}
} // namespace

// gemm_f32_stem.hip (GEMM variant 32)
bool rten_small_c_conv_f32_supported(const rten_hip_conv2d_desc *d, int weights_packed, const float *residual);
int32_t rten_small_c_conv_f32(rten_hip_ctx *ctx, const rten_hip_conv2d_desc *d, const float *x, const float *w_packed, const float *bias, uint32_t flags, float *y);

// depthwise.hip (flags: RTEN_HIP_CONV_RESIDUAL only; the activation is `act`)
int32_t rten_depthwise_conv2d_f32(rten_hip_ctx *ctx, const rten_hip_conv2d_desc *d, const float *x, const float *w, int32_t weights_packed, const float *bias,
                                  const float *residual, uint32_t flags, const RtenAct &act, float *y);

RTEN_EXPORT size_t rten_hip_conv2d_f32_packed_bytes(const rten_hip_conv2d_desc *d) {
    if (!d || d->groups <= 0) return 0;
    const int Og = d->o / d->groups, Og4 = (Og + 3) & ~3;
    const long long K = (long long)(d->c / d->groups) * d->kh * d->kw;
    return (size_t)d->groups * K * Og4 * sizeof(float);
}

RTEN_EXPORT int32_t rten_hip_conv2d_f32_prepack(rten_hip_ctx *ctx, const rten_hip_conv2d_desc *d, const float *w,
                                                float *packed) {
    RTEN_CHECK_CTX(ctx);
    int32_t rc = check_conv_desc(ctx, d);
    if (rc) return rc;
    if (!w || !packed) return RTEN_HIP_ERR_INVALID_VALUE;
    const int Og = d->o / d->groups, Og4 = (Og + 3) & ~3;
    const int K = (d->c / d->groups) * d->kh * d->kw;
    const long long total = (long long)d->groups * K * Og4;
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(conv_prepack_f32_kernel, dim3(blocks), dim3(256), 0, ctx->stream, w, packed, d->groups, Og, K,
                       Og4);
    RTEN_LAUNCH_CHECK(ctx, "conv_prepack_f32_kernel launch");
    return RTEN_HIP_OK;
}

namespace {
// `act`: the epilogue activation (flags' RTEN_HIP_CONV_RELU already folded into it)
int32_t conv2d_f32_impl(rten_hip_ctx *ctx, const rten_hip_conv2d_desc *d, const float *x, const float *w, int32_t weights_packed, const float *bias,
                        const float *residual, uint32_t flags, const RtenAct &act, float *y) {
    int32_t rc = check_conv_desc(ctx, d);
    if (rc) return rc;
    if (!x || !w || !y) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "conv: NULL operand");
    if ((flags & RTEN_HIP_CONV_RESIDUAL) && !residual)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "conv: residual flag without residual tensor");
    if (d->n == 0 || d->out_h == 0 || d->out_w == 0) return RTEN_HIP_OK;
    {   // dispatch order of conv_impl (conv.rs:248-284): the pointwise GEMM first (groups == 1 only), then depthwise
        const bool pw = d->kh == 1 && d->kw == 1 && d->groups == 1 && d->stride_h == 1 && d->stride_w == 1 && d->dil_h == 1 && d->dil_w == 1 &&
                        d->pads[0] == 0 && d->pads[1] == 0 && d->pads[2] == 0 && d->pads[3] == 0;
        if (!pw && d->c == d->o && d->groups == d->c) return rten_depthwise_conv2d_f32(ctx, d, x, w, weights_packed, bias, residual, flags, act, y);
    }
    // the stem kernel's epilogue knows Relu only: other activations take the generic forms
    const uint32_t stem_flags = (flags & ~RTEN_HIP_CONV_RELU) | (act.kind == RTEN_HIP_ACT_RELU ? RTEN_HIP_CONV_RELU : 0u);
    // variant 32 (also what -1 = automatic picks there): 3-channel 7x7 stride-2 convolutions (a ResNet stem) as a direct implicit GEMM over an image patch in LDS
    // (gemm_f32_stem.hip); same bits
    if ((ctx->gemm_variant_override == 32 || ctx->gemm_variant_override < 0) && act.kind <= RTEN_HIP_ACT_RELU && aligned16(w) &&
        rten_small_c_conv_f32_supported(d, weights_packed, (flags & RTEN_HIP_CONV_RESIDUAL) ? residual : nullptr))
        return rten_small_c_conv_f32(ctx, d, x, w, bias, stem_flags, y);
    const int Cg = d->c / d->groups, Og = d->o / d->groups, Og4 = (Og + 3) & ~3;
    const int K = Cg * d->kh * d->kw;
    const int P = d->out_h * d->out_w;
    const long long HW = (long long)d->h * d->w;
    if ((long long)K * Og4 * 4 > kMaxBufBytes)
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "conv: weights above 2 GiB per group are not supported");

    GemmArgs g = {};
    g.A = w; g.B = x; g.C = y; g.bias = bias; g.res = (flags & RTEN_HIP_CONV_RESIDUAL) ? residual : nullptr;
    g.M = Og; g.N = d->n * P; g.K = K;
    int al;
    if (weights_packed) {
        g.a_rs = 1; g.a_cs = Og4; g.a_bs = (long long)K * Og4;
        al = aligned16(w) ? A_M4 : A_SCALAR;
        g.a_dir_m = 1;
        g.a_bytes = (unsigned)((long long)K * Og4 * 4);
    } else {
        g.a_rs = K; g.a_cs = 1; g.a_bs = (long long)Og * K;
        al = A_SCALAR;
        g.a_dir_m = 0;
        g.a_bytes = (unsigned)((long long)Og * K * 4);
    }
    g.b_bs = (long long)Cg * HW;
    g.b_ns = (long long)d->c * HW;
    // one group's slice spans from its first channel of image 0 to its last channel of the last image
    g.b_bytes = (unsigned)((((long long)(d->n - 1) * d->c + Cg) * HW) * 4);
    g.c_rs = P; g.c_ns = (long long)d->o * P; g.c_bs = (long long)Og * P;
    g.bias_bs = Og;
    g.Pn = P;
    g.alpha = 1.f; g.beta = 0.f;
    g.bias_kind = bias ? RTEN_HIP_BIAS_PER_ROW : RTEN_HIP_BIAS_NONE;
    g.act = act.kind; g.act_a = act.alpha; g.act_b = act.beta;

    const bool pointwise = d->kh == 1 && d->kw == 1 && d->stride_h == 1 && d->stride_w == 1 && d->pads[0] == 0 &&
                           d->pads[1] == 0 && d->pads[2] == 0 && d->pads[3] == 0; // conv.rs:250-258 (dilation is moot)
    int bl = B_IM2COL;
    if (pointwise && al == A_M4 && (P % 4) == 0 && aligned16(x)) {
        // the image batch is a two-level [C, (n, H*W)] matrix: no gather needed
        bl = B_N4;
        g.b_rs = HW; g.b_cs = 1;
    } else {
        // <= 31 kernel taps on an LDS-DMA pipeline: per-lane padding bitmask instead of per-gather bounds tests
        const int taps = (al == A_M4 && ctx->pipeline != 0 && d->kh * d->kw <= 31) ? 1 : 0;
        if (taps) bl = B_IM2COL_TAPS;
        g.KH = d->kh; g.KW = d->kw; g.dy = d->dil_h; g.dx = d->dil_w;
        g.lut = get_im2col_lut(ctx, Cg, d->kh, d->kw, d->dil_h, d->dil_w, d->h, d->w, taps);
        if (!g.lut) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "conv: im2col table allocation failed (warm up before graph capture)");
        g.H = d->h; g.W = d->w; g.OW = d->out_w;
        g.sy = d->stride_h; g.sx = d->stride_w;
        g.pt = d->pads[0]; g.pl = d->pads[1];
    }
    g.b_dir_n = 1;
    g.debug = ctx->debug;
    return dispatch(ctx, g, d->groups, al, bl);
}
} // namespace

RTEN_EXPORT int32_t rten_hip_conv2d_f32(rten_hip_ctx *ctx, const rten_hip_conv2d_desc *d, const float *x, const float *w,
                                        int32_t weights_packed, const float *bias, const float *residual,
                                        uint32_t flags, float *y) {
    RTEN_CHECK_CTX(ctx);
    const RtenAct act = {(flags & RTEN_HIP_CONV_RELU) ? RTEN_HIP_ACT_RELU : RTEN_HIP_ACT_NONE, 0.f, 0.f};
    return conv2d_f32_impl(ctx, d, x, w, weights_packed, bias, residual, flags, act, y);
}

RTEN_EXPORT int32_t rten_hip_conv2d_f32_act(rten_hip_ctx *ctx, const rten_hip_conv2d_desc *d, const float *x, const float *w,
                                            int32_t weights_packed, const float *bias, const float *residual,
                                            uint32_t flags, int32_t act_kind, float act_alpha, float act_beta, float *y) {
    RTEN_CHECK_CTX(ctx);
    if (flags & RTEN_HIP_CONV_RELU) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "conv_act: pass Relu as the activation, not as a flag");
    if (!rten_act_valid(act_kind)) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "conv_act: unknown activation kind");
    const RtenAct act = {act_kind, act_alpha, act_beta};
    return conv2d_f32_impl(ctx, d, x, w, weights_packed, bias, residual, flags, act, y);
}

#ifdef RTEN_TRACE
RtenTraceHost g_trace_host;
// Trace builds only: hand the kernels a device buffer of `cap` 128-byte records (NULL: off) / read the number of record slots handed out to launches so far.
RTEN_EXPORT int32_t rten_hip_debug_trace_set(rten_hip_ctx *ctx, void *buf, uint32_t cap) {
    RTEN_CHECK_CTX(ctx);
    g_trace_host.buf = (unsigned long long *)buf;
    g_trace_host.cap = cap;
    return RTEN_HIP_OK;
}
RTEN_EXPORT int32_t rten_hip_debug_trace_count(rten_hip_ctx *ctx, uint32_t *n) {
    RTEN_CHECK_CTX(ctx);
    *n = g_trace_host.next;
    return RTEN_HIP_OK;
}
#endif
