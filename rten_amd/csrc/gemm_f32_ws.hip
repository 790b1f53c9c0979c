// The wave-specialised family of the f32 implicit-GEMM kernels (gfx950): four MFMA waves + four loader waves per workgroup on the LDS-DMA
// ring (pipeline 2, GEMM variants 8..11).  Prepacked (k-major) weights only; no split-K form.  Launch plans: gemm_f32.hip.
#include "gemm_f32_common.h"

namespace {

template <int BM, int BN, int BL, bool MULTI_KC>
__global__ __launch_bounds__(2 * NTHREADS, 2) void igemm_f32_ws_kernel(const GemmArgs p) {
    kernarg_prefetch<(int)sizeof(GemmArgs)>();
    static_assert(BL == B_N4 || BL == B_IM2COL || BL == B_IM2COL_TAPS, "DMA kernel covers the conv operand layouts");
    constexpr int WM = 2, WN = 2;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int STAGE = BK * (BM + BN); // floats per stage
    constexpr int NA = BK * BM / 256 / 4; // dwordx4 DMA instructions per wave per tile (A)
    constexpr int NBV = BK * BN / 256 / 4; // dwordx4 (dense B)
    constexpr int NBG = BK * BN / 64 / 4;  // dword gathers per wave per tile (im2col B)
    constexpr int PER_TILE = NA + (BL == B_N4 ? NBV : NBG);
    static_assert(NA >= 1 && NBV >= 1, "tile too small for 4-wave DMA split");
    constexpr int NSTAGE = 3; // (deeper rings measured slower: LDS-limited occupancy, no gain for a lone workgroup)
    __shared__ __attribute__((aligned(16))) float smem[NSTAGE * STAGE];

    // 8 waves: 0..3 multiply (one per SIMD), 4..7 are loader waves that only issue LDS-DMA.  The two roles share
    // each SIMD, so address arithmetic / DMA issue of the loader overlaps the MFMA wave's matrix-pipe time even
    // when this is the only workgroup on the CU.
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool is_loader = wave_all >= 4;
    const int wave = wave_all & 3; // loader index or MFMA wave index
    const int l31 = lane & 31, half = lane >> 5;
    const int z = blockIdx.y;

    const int tile = xcd_chunked_tile(blockIdx.x, p.tiles_m * p.tiles_n);
    const int bm = (p.order & 1) ? tile / p.tiles_n : tile % p.tiles_m, bn = (p.order & 1) ? tile % p.tiles_n : tile / p.tiles_m;
    const int m0 = bm * BM, n0 = bn * BN;

    const BatchSlice zs = batch_slice(p, z);
    const long long c_zoff = zs.c_zoff;
    const __amdgpu_buffer_rsrc_t rsA = slice_rsrc(zs.A, p.a_bytes), rsB = slice_rsrc(zs.B, p.b_bytes);
    const int nk = (p.K + BK - 1) / BK;

    // ---- loop-invariant DMA source offsets.  Wave w issues instructions q = w*N + j; instruction q covers
    // the flat tile range [q*256, q*256+256) floats (dwordx4) or [q*64, q*64+64) (dword gather).
    unsigned a_voff[NA];
    dma_a_offsets_m4<BM, NA>(p, m0, wave, lane, a_voff);
    const unsigned a_kstep = (unsigned)(BK * p.a_cs * 4);

    [[maybe_unused]] unsigned b_voff[BL == B_N4 ? NBV : 1];
    [[maybe_unused]] int b_krow[BL == B_N4 ? NBV : 1];
    [[maybe_unused]] unsigned b_kstep = 0;
    constexpr bool IM2COL = BL == B_IM2COL || BL == B_IM2COL_TAPS, TAPS = BL == B_IM2COL_TAPS;
    constexpr int NCOL = IM2COL && BN == 128 ? 2 : 1;
    [[maybe_unused]] int im_iy0[NCOL], im_ix0[NCOL], im_pix[NCOL];
    [[maybe_unused]] unsigned im_inv[NCOL]; // TAPS: bit t set = tap t of this lane's pixel is padding; bit 31 always set (k-tail rows)
    if constexpr (BL == B_N4) {
        dma_b_offsets<BN, NBV>(p, n0, wave, lane, b_voff, b_krow);
        b_kstep = (unsigned)(BK * p.b_rs * 4);
    } else {
#pragma unroll
        for (int c = 0; c < BN / 64; c++) // a lane sees one column per 64 of the tile
            im2col_column<TAPS>(p, n0 + c * 64 + lane, im_iy0[c], im_ix0[c], im_pix[c], im_inv[c]);
    }

    // im2col LUT entries (scalar loads) for the tile whose DMA is issued NEXT
    typedef const __attribute__((address_space(4))) i32x2 *lut_ptr_t;
    constexpr int LROWS = BK / 4; // rows of a tile handled by one wave (NBG / (BN/64))
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
        const int kts = kt < nk ? kt : (nk > 0 ? nk - 1 : 0); // keep the scalar offset inside the buffer
        const bool past = kt >= nk;
        const unsigned a_soff = (unsigned)kts * a_kstep;
#pragma unroll
        for (int j = 0; j < NA; j++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_t)(As + (wave * NA + j) * 256), 16,
                                                     (int)(past ? OOB : a_voff[j]), (int)a_soff, 0, 0);
        if constexpr (BL == B_N4) {
            const int kleft = p.K - kt * BK;
            const unsigned b_soff = (unsigned)kts * b_kstep;
#pragma unroll
            for (int j = 0; j < NBV; j++)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr_t)(Bs + (wave * NBV + j) * 256), 16,
                                                         (int)(b_krow[j] < kleft ? b_voff[j] : OOB), (int)b_soff, 0, 0);
        } else {
#pragma unroll
            for (int j = 0; j < NBG; j++) {
                constexpr int CPR = BN / 64;            // gather instructions per tile row
                const int r = j / CPR, c = j % CPR;     // row within this wave's LROWS, column chunk
                const i32x2 e = lutE[r];
                unsigned voff;
                if constexpr (TAPS) {
                    // e[1] = 31 - tap: the tap's padding bit moves to bit 31 and pushes the offset out of range
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

    // ---- accumulators / epilogue helpers (same numerics as igemm_f32_kernel)
    const int wq = (t >> 6) & 3; // per-lane copy of the MFMA wave id for address math
    const int wm0 = (wq / WN) * (BM / WM), wn0 = (wq % WN) * (BN / WN);
    f32x16 acc[TM][TN];
    [[maybe_unused]] f32x16 tot[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
    [[maybe_unused]] auto flush = [&](bool first) {
        int mb = m0 + wm0 + 4 * half, nb0 = n0 + wn0 + l31;
        asm volatile("" : "+v"(mb), "+v"(nb0));
        if (first) fold_first<TM, TN>(p, z, acc, tot, mb, nb0, c_zoff);
        else fold_next<TM, TN>(p, acc, tot);
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
    };

    auto compute_tile = [&](int stage) {
        const float *As = smem + stage * STAGE + wm0 + l31;
        const float *Bs = smem + stage * STAGE + BK * BM + wn0 + l31;
        float af[2][TM], bf[2][TN]; // operand fragments, double buffered across k-pairs
#pragma unroll
        for (int i = 0; i < TM; i++) af[0][i] = As[half * BM + i * 32];
#pragma unroll
        for (int j = 0; j < TN; j++) bf[0][j] = Bs[half * BN + j * 32];
#pragma unroll
        for (int kk = 0; kk < BK / 2; kk++) {
            const int cur = kk & 1, nxt = cur ^ 1;
            if (kk + 1 < BK / 2) {
#pragma unroll
                for (int i = 0; i < TM; i++) af[nxt][i] = As[(2 * (kk + 1) + half) * BM + i * 32];
#pragma unroll
                for (int j = 0; j < TN; j++) bf[nxt][j] = Bs[(2 * (kk + 1) + half) * BN + j * 32];
            }
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < TN; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_iglp_opt(0); // interleave the next group's ds_reads behind the current group's first MFMA
    };

    // ---- software pipeline: tiles kt+1 and kt+2 are in flight while tile kt is multiplied.  One s_barrier per
    // k-tile, executed by all 8 waves: loaders arrive after their DMA of tile kt has landed, MFMA waves after they
    // finished tile kt-1; past the barrier the loaders refill the freed stage while the MFMA waves multiply.
    const int nblk = MULTI_KC ? (nk + KC_TILES - 1) / KC_TILES : 1;
    if (is_loader) {
        fetch_lut(0);
#pragma unroll
        for (int i = 0; i < NSTAGE - 1; i++) {
            issue_tile(i, i);
            fetch_lut(i + 1);
        }
        int stage = 0;
        for (int kt = 0; kt < nk; kt++) {
            wait_vmcnt<PER_TILE *(NSTAGE - 2)>();
            __builtin_amdgcn_s_barrier();
            const int stp = stage == 0 ? NSTAGE - 1 : stage - 1;
            if (!(ABLATE(p) & 1)) issue_tile(kt + NSTAGE - 1, stp);
            fetch_lut(kt + NSTAGE);
            stage = stage == NSTAGE - 1 ? 0 : stage + 1;
        }
        wait_vmcnt<0>(); // the look-ahead tiles (out of range, zero fill) must land before the LDS goes away
        return;
    }
    {
        int stage = 0;
        for (int blk = 0; blk < nblk; blk++) {
            const int kt_end = MULTI_KC ? ((blk + 1) * KC_TILES < nk ? (blk + 1) * KC_TILES : nk) : nk;
            for (int kt = blk * KC_TILES; kt < kt_end; kt++) {
                __builtin_amdgcn_s_barrier();
                if (!(ABLATE(p) & 2)) compute_tile(stage);
                stage = stage == NSTAGE - 1 ? 0 : stage + 1;
            }
            if constexpr (MULTI_KC) {
                if (blk + 1 < nblk) flush(blk == 0);
            }
        }
    }

    if (!(ABLATE(p) & 4)) {
        const int mb = m0 + wm0 + 4 * half, nb0 = n0 + wn0 + l31;
        if constexpr (MULTI_KC) { // launched only for K > 256: at least two depth blocks
            fold_next<TM, TN>(p, acc, tot);
            store_out<TM, TN, false>(p, tot, mb, nb0, c_zoff); // (acc and tot live: no room for the activations past Gelu, see launch_cfg)
        } else {
            fold_first<TM, TN>(p, z, acc, acc, mb, nb0, c_zoff);
            store_out<TM, TN>(p, acc, mb, nb0, c_zoff);
        }
    }
}

template <int BM, int BN, int BL>
int32_t launch(rten_hip_ctx *ctx, const GemmArgs &a, dim3 grid, int mode, double flops, double bytes) {
    char kname[96];
    snprintf(kname, sizeof kname, "igemm_f32_ws_kernel<%d,%d,%d,%s>", BM, BN, BL, mode == 1 ? "true" : "false");
    ProfScope ps(ctx, kname, flops, bytes);
    if (mode == 1) hipLaunchKernelGGL((igemm_f32_ws_kernel<BM, BN, BL, true>), grid, dim3(2 * NTHREADS), 0, ctx->stream, a);
    else hipLaunchKernelGGL((igemm_f32_ws_kernel<BM, BN, BL, false>), grid, dim3(2 * NTHREADS), 0, ctx->stream, a);
    RTEN_LAUNCH_CHECK(ctx, "igemm_f32_ws_kernel launch");
    return RTEN_HIP_OK;
}

} // namespace

int32_t rten_launch_gemm_f32_ws(rten_hip_ctx *ctx, const void *args, unsigned grid_x, unsigned grid_z, int bm, int bn, int bl, int mode, double flops,
                                double bytes) {
    TRACED_ARGS(a, args, grid_x * grid_z);
    const dim3 grid(grid_x, grid_z);
    return switch_tile(ctx, "igemm_f32_ws_kernel", bm, bn, [&](auto t) -> int32_t {
        constexpr int BM = decltype(t)::bm, BN = decltype(t)::bn;
        switch (bl) {
        case B_N4: return launch<BM, BN, B_N4>(ctx, a, grid, mode, flops, bytes);
        case B_IM2COL: return launch<BM, BN, B_IM2COL>(ctx, a, grid, mode, flops, bytes);
        case B_IM2COL_TAPS: return launch<BM, BN, B_IM2COL_TAPS>(ctx, a, grid, mode, flops, bytes);
        default: return not_covered(ctx, "igemm_f32_ws_kernel");
        }
    });
}
