// The 16x16x4 family of the f32 implicit-GEMM kernels (gfx950): the LDS-DMA pipeline on v_mfma_f32_16x16x4_f32 (pipeline 5, GEMM
// variants 20..23).  Its fold / epilogue (fold_first16, fold_next16, store_out16) lives in gemm_f32_common.h.  Launch plans: gemm_f32.hip.
#include "gemm_f32_common.h"

namespace {

// =====================================================================================================
// LDS-DMA kernel on v_mfma_f32_16x16x4_f32: the same tile DMA, LDS image and depth-block fold as igemm_f32_dma_kernel, but a
// wave's (BM/2) x (BN/2) share is a grid of 16x16 accumulator blocks.  With 64x64 tiles the 32x32x2 form leaves every wave ONE
// accumulator, i.e. a chain of dependent MFMAs: whatever the wave issues between two of them (the next operands' ds_reads) costs
// ~43 cycles beyond its own slot, and the dependent latency itself is the whole 64-cycle issue time.  Four independent 16x16
// accumulators (40-cycle dependent latency, revisited every 128 cycles) take both stalls away at the same LDS traffic per flop.
// v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain (tools/probes/mfma_16x16x4_order.hip): same bits.  MODE 0 / 1 (no split-K form).
// Accumulator element r of block (i, j): row wm0 + 16 i + 4 * (lane / 16) + r, column wn0 + 16 j + lane % 16.
// =====================================================================================================
template <int BM, int BN, int AL, int BL, int MODE>
__global__ __launch_bounds__(NTHREADS, 2) void igemm_f32_dma16_kernel(const GemmArgs p) {
    kernarg_prefetch<(int)sizeof(GemmArgs)>();
    constexpr bool MULTI_KC = MODE == 1;
    static_assert(MODE == 0 || MODE == 1, "the 16x16x4 kernel has no split-K form");
    static_assert(AL == A_M4 || AL == A_K4, "DMA kernel: A is k-major or row-major with 16-byte rows");
    static_assert(BL == B_N4 || BL == B_IM2COL || BL == B_IM2COL_TAPS, "DMA kernel covers the conv operand layouts");
    constexpr int WM = 2, WN = 2;
    constexpr int TM2 = BM / WM / 16, TN2 = BN / WN / 16;
    constexpr int STAGE = BK * (BM + BN);
    constexpr int NA = BK * BM / 256 / 4;
    constexpr int NBV = BK * BN / 256 / 4;
    constexpr int NBG = BK * BN / 64 / 4;
    constexpr int PER_TILE = NA + (BL == B_N4 ? NBV : NBG);
    constexpr int NSTAGE = 3;
    __shared__ __attribute__((aligned(16))) float smem[NSTAGE * STAGE];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, quad = lane >> 4;
    const int z = blockIdx.y;

    const int tile = xcd_chunked_tile(blockIdx.x, (int)gridDim.x);
    const int bm = (p.order & 1) ? tile / p.tiles_n : tile % p.tiles_m, bn = (p.order & 1) ? tile % p.tiles_n : tile / p.tiles_m;
    const int m0 = bm * BM, n0 = bn * BN;

    const BatchSlice zs = batch_slice(p, z);
    const long long c_zoff = zs.c_zoff;
    const __amdgpu_buffer_rsrc_t rsA = slice_rsrc(zs.A, p.a_bytes), rsB = slice_rsrc(zs.B, p.b_bytes);
    const int nk = (p.K + BK - 1) / BK;

    unsigned a_voff[NA];
    [[maybe_unused]] int a_kq[NA];
    dma_a_offsets<BM, AL, NA>(p, m0, wave, lane, a_voff, a_kq);
    const unsigned a_kstep = AL == A_M4 ? (unsigned)(BK * p.a_cs * 4) : (unsigned)(BK * 4);

    [[maybe_unused]] unsigned b_voff[BL == B_N4 ? NBV : 1];
    [[maybe_unused]] int b_krow[BL == B_N4 ? NBV : 1];
    [[maybe_unused]] unsigned b_kstep = 0;
    constexpr bool IM2COL = BL == B_IM2COL || BL == B_IM2COL_TAPS, TAPS = BL == B_IM2COL_TAPS;
    constexpr int NCOL = IM2COL && BN == 128 ? 2 : 1;
    [[maybe_unused]] int im_iy0[NCOL], im_ix0[NCOL], im_pix[NCOL];
    [[maybe_unused]] unsigned im_inv[NCOL];
    if constexpr (BL == B_N4) {
        dma_b_offsets<BN, NBV>(p, n0, wave, lane, b_voff, b_krow);
        b_kstep = (unsigned)(BK * p.b_rs * 4);
    } else {
#pragma unroll
        for (int c = 0; c < BN / 64; c++) // a lane sees one column per 64 of the tile
            im2col_column<TAPS>(p, n0 + c * 64 + lane, im_iy0[c], im_ix0[c], im_pix[c], im_inv[c]);
    }

    typedef const __attribute__((address_space(4))) i32x2 *lut_ptr_t;
    constexpr int LROWS = BK / 4;
    [[maybe_unused]] i32x2 lutE[LROWS];
    [[maybe_unused]] auto fetch_lut = [&](int kt) {
        if constexpr (IM2COL) {
            const int krow0 = kt * BK + wave * LROWS;
            const lut_ptr_t lc = (lut_ptr_t)(unsigned long long)p.lut;
#pragma unroll
            for (int j = 0; j < LROWS; j++) lutE[j] = lc[krow0 + j];
        }
    };

    typedef __attribute__((address_space(3))) void *lds_ptr_t;
    auto issue_tile = [&](int kt, int stage) {
        float *As = smem + stage * STAGE;
        float *Bs = As + BK * BM;
        const int kts = kt < nk ? kt : (nk > 0 ? nk - 1 : 0);
        const bool past = kt >= nk;
        const unsigned a_soff = (unsigned)kts * a_kstep;
#pragma unroll
        for (int j = 0; j < NA; j++) {
            bool dead = past;
            if constexpr (AL == A_K4) dead = a_kq[j] >= p.K - kt * BK;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_t)(As + (wave * NA + j) * 256), 16, (int)(dead ? OOB : a_voff[j]), (int)a_soff, 0, 0);
        }
        if constexpr (BL == B_N4) {
            const int kleft = p.K - kt * BK;
            const unsigned b_soff = (unsigned)kts * b_kstep;
#pragma unroll
            for (int j = 0; j < NBV; j++)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr_t)(Bs + (wave * NBV + j) * 256), 16, (int)(b_krow[j] < kleft ? b_voff[j] : OOB), (int)b_soff, 0, 0);
        } else {
#pragma unroll
            for (int j = 0; j < NBG; j++) {
                constexpr int CPR = BN / 64;
                const int r = j / CPR, c = j % CPR;
                const i32x2 e = lutE[r];
                unsigned voff;
                if constexpr (TAPS) {
                    voff = ((im_inv[c] << e[1]) & 0x80000000u) | ((unsigned)(im_pix[c] + e[0]) << 2);
                } else {
                    const int iy = im_iy0[c] + (e[1] & 0xffff);
                    const int ix = im_ix0[c] + (e[1] >> 16);
                    const bool ok = ((unsigned)iy < (unsigned)p.H) & ((unsigned)ix < (unsigned)p.W);
                    voff = ok ? (unsigned)(im_pix[c] + e[0]) << 2 : OOB;
                }
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr_t)(Bs + (wave * LROWS + r) * BN + c * 64), 4, (int)voff, 0, 0, 0);
            }
        }
    };

    const int wq = t >> 6;
    const int wm0 = (wq / WN) * (BM / WM), wn0 = (wq % WN) * (BN / WN);
    f32x4v acc[TM2][TN2];
    [[maybe_unused]] f32x4v tot[TM2][TN2];
#pragma unroll
    for (int i = 0; i < TM2; i++)
#pragma unroll
        for (int j = 0; j < TN2; j++) acc[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] auto flush = [&](bool first) {
        int mb = m0 + wm0 + 4 * quad, nb0 = n0 + wn0 + l15;
        asm volatile("" : "+v"(mb), "+v"(nb0));
        if (first) fold_first16<TM2, TN2>(p, z, acc, tot, mb, nb0, c_zoff);
        else fold_next16<TM2, TN2>(p, acc, tot);
#pragma unroll
        for (int i = 0; i < TM2; i++)
#pragma unroll
            for (int j = 0; j < TN2; j++) acc[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};
    };

    auto compute_tile = [&](int stage) {
        // k-step ks covers rows 4 ks .. 4 ks + 3 of the tile; lane -> k = 4 ks + quad.  k-major image As[k][m]; row-major image [k/4][m][4]
        const float *As = smem + stage * STAGE + (AL == A_M4 ? wm0 + l15 + quad * BM : (wm0 + l15) * 4 + quad);
        auto a_idx = [](int ks, int i) { return AL == A_M4 ? 4 * ks * BM + i * 16 : ks * BM * 4 + i * 64; };
        const float *Bs = smem + stage * STAGE + BK * BM + wn0 + l15 + quad * BN;
        float af[2][TM2], bf[2][TN2];
#pragma unroll
        for (int i = 0; i < TM2; i++) af[0][i] = As[a_idx(0, i)];
#pragma unroll
        for (int j = 0; j < TN2; j++) bf[0][j] = Bs[j * 16];
#pragma unroll
        for (int ks = 0; ks < BK / 4; ks++) {
            const int cur = ks & 1, nxt = cur ^ 1;
            if (ks + 1 < BK / 4) {
#pragma unroll
                for (int i = 0; i < TM2; i++) af[nxt][i] = As[a_idx(ks + 1, i)];
#pragma unroll
                for (int j = 0; j < TN2; j++) bf[nxt][j] = Bs[4 * (ks + 1) * BN + j * 16];
            }
#pragma unroll
            for (int i = 0; i < TM2; i++)
#pragma unroll
                for (int j = 0; j < TN2; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_iglp_opt(0);
    };

    const int nblk = MULTI_KC ? (nk + KC_TILES - 1) / KC_TILES : 1;
    fetch_lut(0);
#pragma unroll
    for (int i = 0; i < NSTAGE - 1; i++) {
        issue_tile(i, i);
        fetch_lut(i + 1);
    }
    int stage = 0;
    for (int blk = 0; blk < nblk; blk++) {
        const int kt_end = MULTI_KC ? ((blk + 1) * KC_TILES < nk ? (blk + 1) * KC_TILES : nk) : nk;
        for (int kt = blk * KC_TILES; kt < kt_end; kt++) {
            wait_vmcnt<PER_TILE *(NSTAGE - 2)>();
            __builtin_amdgcn_s_barrier();
            const int stp = stage == 0 ? NSTAGE - 1 : stage - 1;
            issue_tile(kt + NSTAGE - 1, stp);
            fetch_lut(kt + NSTAGE);
            compute_tile(stage);
            stage = stage == NSTAGE - 1 ? 0 : stage + 1;
        }
        if constexpr (MULTI_KC) {
            if (blk + 1 < nblk) flush(blk == 0);
        }
    }
    wait_vmcnt<0>();

    const int mb = m0 + wm0 + 4 * quad, nb0 = n0 + wn0 + l15;
    if constexpr (MULTI_KC) {
        fold_next16<TM2, TN2>(p, acc, tot);
        store_out16<TM2, TN2>(p, tot, mb, nb0, c_zoff);
    } else {
        fold_first16<TM2, TN2>(p, z, acc, acc, mb, nb0, c_zoff);
        store_out16<TM2, TN2>(p, acc, mb, nb0, c_zoff);
    }
}

template <int BM, int BN, int AL, int BL>
int32_t launch(rten_hip_ctx *ctx, const GemmArgs &a, dim3 grid, int mode, double flops, double bytes) {
    char kname[96];
    snprintf(kname, sizeof kname, "igemm_f32_dma16_kernel<%d,%d,%d,%d,%d>", BM, BN, AL, BL, mode);
    ProfScope ps(ctx, kname, flops, bytes);
    if (mode == 1) hipLaunchKernelGGL((igemm_f32_dma16_kernel<BM, BN, AL, BL, 1>), grid, dim3(NTHREADS), 0, ctx->stream, a);
    else hipLaunchKernelGGL((igemm_f32_dma16_kernel<BM, BN, AL, BL, 0>), grid, dim3(NTHREADS), 0, ctx->stream, a);
    RTEN_LAUNCH_CHECK(ctx, "igemm_f32_dma16_kernel launch");
    return RTEN_HIP_OK;
}

} // namespace

int32_t rten_launch_gemm_f32_dma16(rten_hip_ctx *ctx, const void *args, unsigned grid_x, unsigned grid_z, int bm, int bn, int al, int bl, int mode,
                                   double flops, double bytes) {
    TRACED_ARGS(a, args, grid_x * grid_z);
    const dim3 grid(grid_x, grid_z);
    return switch_tile(ctx, "igemm_f32_dma16_kernel", bm, bn, [&](auto t) -> int32_t {
        constexpr int BM = decltype(t)::bm, BN = decltype(t)::bn;
        switch (layouts(al, bl)) {
        case layouts(A_M4, B_N4): return launch<BM, BN, A_M4, B_N4>(ctx, a, grid, mode, flops, bytes);
        case layouts(A_M4, B_IM2COL): return launch<BM, BN, A_M4, B_IM2COL>(ctx, a, grid, mode, flops, bytes);
        case layouts(A_M4, B_IM2COL_TAPS): return launch<BM, BN, A_M4, B_IM2COL_TAPS>(ctx, a, grid, mode, flops, bytes);
        case layouts(A_K4, B_N4): return launch<BM, BN, A_K4, B_N4>(ctx, a, grid, mode, flops, bytes);
        default: return not_covered(ctx, "igemm_f32_dma16_kernel");
        }
    });
}
