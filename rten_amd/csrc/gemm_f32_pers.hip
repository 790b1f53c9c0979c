// The persistent family of the f32 implicit-GEMM kernels (gfx950): split mode 5.  The 16x16x4 fold / epilogue of its MF16 form lives in
// gemm_f32_common.h.  Launch plans: gemm_f32.hip.
#include "gemm_f32_common.h"

namespace {

// =====================================================================================================
// Persistent LDS-DMA kernel: a workgroup walks a LIST of tiles and its tile DMA runs two k-tiles ahead ACROSS tile boundaries.
//
// Why: a pure MFMA stream sustains 154.7 TFLOP/s on this chip (tools/probes/mfma_sustained.hip: 2381 MHz under load), yet the
// one-tile-per-workgroup kernels (gemm_f32_dma.hip) reach 80-105 on ResNet's layers.  Their tiles are short (K = 64 ... 576: 7 us of matrix
// work) and every workgroup starts with ~2 us of load latency and ends with an epilogue that waits on its residual loads and
// stores; all resident workgroups of a CU begin together and stay in lockstep, so those phases do not overlap anybody's MFMAs,
// and the partial last round costs a whole tile latency.  Here a CU's resident workgroups live for the whole launch:
//   * the loader (same DMA instructions, same LDS ring) keeps its own (tile, k-tile) position and simply continues into the next
//     tile of the list, recomputing its per-lane source offsets when it crosses -- the first k-tiles of tile i+1 land while tile
//     i's last MFMAs and epilogue run: no load bubble between tiles;
//   * the launch-time prologue (kernarg loads, LUT warm-up, first DMA latency) is paid once per workgroup, not once per tile;
//   * the grid is num_cus x R workgroups (R = split `groups` of plan mode 5), tiles are dealt round-robin inside each XCD's
//     contiguous chunk (same L2 locality as xcd_chunked_tile's remapped ids).
// Numerics: per output element exactly the chain of the other kernels (k-ordered MFMA chain per depth block of 256, blocks
// folded with separate adds, bias after the first block): bit-identical.  MF16 selects v_mfma_f32_16x16x4_f32 blocks.
// =====================================================================================================
template <int BM, int BN, int AL, int BL, bool MF16, int MFK = 0>
__global__ __launch_bounds__(NTHREADS, (BM * BN >= 128 * 128) ? 1 : 2) void igemm_f32_pers_kernel(const GemmArgs p) {
    kernarg_prefetch<(int)sizeof(GemmArgs)>();
    static_assert(AL == A_M4 || AL == A_K4, "DMA kernel: A is k-major or row-major with 16-byte rows");
    static_assert(BL == B_N4 || BL == B_IM2COL || BL == B_IM2COL_TAPS, "DMA kernel covers the conv operand layouts");
    constexpr int WM = 2, WN = 2;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;    // 32x32 blocks per wave
    constexpr int TM2 = BM / WM / 16, TN2 = BN / WN / 16;  // 16x16 blocks per wave
    constexpr int STAGE = BK * (BM + BN);
    constexpr int NA = BK * BM / 256 / 4;
    constexpr int NBV = BK * BN / 256 / 4;
    constexpr int NBG = BK * BN / 64 / 4;
    constexpr int PER_TILE = NA + (BL == B_N4 ? NBV : NBG);
    constexpr int NSTAGE = 3;
    constexpr bool IM2COL = BL == B_IM2COL || BL == B_IM2COL_TAPS, TAPS = BL == B_IM2COL_TAPS;
    constexpr int NCOL = IM2COL && BN == 128 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float smem[NSTAGE * STAGE];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int z = blockIdx.y;

    // ---- this workgroup's tile list: XCD x = id & 7 owns the contiguous chunk [lo, lo + cnt) of the launch's tiles (as the
    // remapped ids of the one-tile kernels), its workgroups j = id >> 3 take tiles lo + j, lo + j + gx, ...
    const int T = p.tiles_m * p.tiles_n;
    int t_next, t_end, t_step;
    {
        const int id = blockIdx.x, G = (int)gridDim.x;
        const int xcd = id & 7, q = T >> 3, r = T & 7;
        const int lo = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        const int cnt = q + (xcd < r ? 1 : 0);
        t_step = (G - xcd + 7) >> 3; // workgroups on this XCD
        t_next = lo + (id >> 3);
        t_end = lo + cnt;
    }
    if (t_next >= t_end) return; // more workgroups than tiles on this XCD (uniform per workgroup: no barrier is skipped by part of it)

    const BatchSlice zs = batch_slice(p, z);
    const long long c_zoff = zs.c_zoff;
    const __amdgpu_buffer_rsrc_t rsA = slice_rsrc(zs.A, p.a_bytes), rsB = slice_rsrc(zs.B, p.b_bytes);
    const int nk = (p.K + BK - 1) / BK;
    const unsigned a_kstep = AL == A_M4 ? (unsigned)(BK * p.a_cs * 4) : (unsigned)(BK * 4);
    const unsigned b_kstep = BL == B_N4 ? (unsigned)(BK * p.b_rs * 4) : 0u;

    // ---- loader state: position (l_tile, l_kt) in this workgroup's stream of k-tiles and the per-lane source offsets of l_tile
    int l_tile = t_next, l_kt = 0;
    bool l_dead = false; // past the last tile of the list: the ring keeps turning on zero-fill loads
    unsigned a_voff[NA];
    [[maybe_unused]] int a_kq[NA];
    [[maybe_unused]] unsigned b_voff[BL == B_N4 ? NBV : 1];
    [[maybe_unused]] int b_krow[BL == B_N4 ? NBV : 1];
    [[maybe_unused]] int im_iy0[NCOL], im_ix0[NCOL], im_pix[NCOL];
    [[maybe_unused]] unsigned im_inv[NCOL];
    auto tile_origin = [&](int tile, int &m0, int &n0) {
        const int bm = (p.order & 1) ? tile / p.tiles_n : tile % p.tiles_m, bn = (p.order & 1) ? tile % p.tiles_n : tile / p.tiles_m;
        m0 = bm * BM;
        n0 = bn * BN;
    };
    auto setup_loader = [&](int tile) {
        int m0, n0;
        tile_origin(tile, m0, n0);
        dma_a_offsets<BM, AL, NA>(p, m0, wave, lane, a_voff, a_kq);
        if constexpr (BL == B_N4) {
            dma_b_offsets<BN, NBV>(p, n0, wave, lane, b_voff, b_krow);
        } else {
#pragma unroll
            for (int c = 0; c < BN / 64; c++) // a lane sees one column per 64 of the tile
                im2col_column<TAPS>(p, n0 + c * 64 + lane, im_iy0[c], im_ix0[c], im_pix[c], im_inv[c]);
        }
    };

    typedef const __attribute__((address_space(4))) i32x2 *lut_ptr_t;
    constexpr int LROWS = BK / 4;
    [[maybe_unused]] i32x2 lutE[LROWS];
    [[maybe_unused]] auto fetch_lut = [&](int kt) { // LUT rows of the k-tile the loader issues NEXT (one table per conv geometry: tile independent)
        if constexpr (IM2COL) {
            const int krow0 = kt * BK + wave * LROWS;
            const lut_ptr_t lc = (lut_ptr_t)(unsigned long long)p.lut;
#pragma unroll
            for (int j = 0; j < LROWS; j++) lutE[j] = lc[krow0 + j];
        }
    };

    typedef __attribute__((address_space(3))) void *lds_ptr_t;
    auto issue_tile = [&](int stage) { // DMA of (l_tile, l_kt) into `stage`, then advance the loader
        float *As = smem + stage * STAGE;
        float *Bs = As + BK * BM;
        const int kt = l_kt;
        const unsigned a_soff = (unsigned)kt * a_kstep;
#pragma unroll
        for (int j = 0; j < NA; j++) {
            bool dead = l_dead;
            if constexpr (AL == A_K4) dead = dead || a_kq[j] >= p.K - kt * BK;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_t)(As + (wave * NA + j) * 256), 16, (int)(dead ? OOB : a_voff[j]), (int)(l_dead ? 0u : a_soff), 0, 0);
        }
        if constexpr (BL == B_N4) {
            const int kleft = p.K - kt * BK;
            const unsigned b_soff = (unsigned)kt * b_kstep;
#pragma unroll
            for (int j = 0; j < NBV; j++)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr_t)(Bs + (wave * NBV + j) * 256), 16,
                                                         (int)((!l_dead && b_krow[j] < kleft) ? b_voff[j] : OOB), (int)(l_dead ? 0u : b_soff), 0, 0);
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
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr_t)(Bs + (wave * LROWS + r) * BN + c * 64), 4, (int)(l_dead ? OOB : voff), 0, 0, 0);
            }
        }
        // advance: next k-tile of this tile, or the first k-tile of the next tile of the list (new per-lane offsets)
        if (!l_dead) {
            if (++l_kt == nk) {
                l_kt = 0;
                l_tile += t_step;
                if (l_tile < t_end) setup_loader(l_tile);
                else l_dead = true;
            }
        }
        fetch_lut(l_kt);
    };

    // ---- accumulators
    const int wq = t >> 6;
    const int wm0 = (wq / WN) * (BM / WM), wn0 = (wq % WN) * (BN / WN);
    const int l31 = lane & 31, half = lane >> 5, l15 = lane & 15, quad = lane >> 4;
    f32x16 acc[MF16 ? 1 : TM][MF16 ? 1 : TN], tot[MF16 ? 1 : TM][MF16 ? 1 : TN];
    f32x4v acc4[MF16 ? TM2 : 1][MF16 ? TN2 : 1], tot4[MF16 ? TM2 : 1][MF16 ? TN2 : 1];
    auto zero_acc = [&]() {
        if constexpr (MF16) {
#pragma unroll
            for (int i = 0; i < TM2; i++)
#pragma unroll
                for (int j = 0; j < TN2; j++) acc4[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < TN; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
        }
    };

    auto compute_tile = [&](int stage) {
        if constexpr (MF16) {
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
                    for (int j = 0; j < TN2; j++) acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[cur][i], bf[cur][j], acc4[i][j], 0, 0, 0);
            }
        } else {
            const float *As = smem + stage * STAGE + (AL == A_M4 ? wm0 + l31 + half * BM : (wm0 + l31) * 4 + half);
            auto a_idx = [](int kk, int i) { return AL == A_M4 ? 2 * kk * BM + i * 32 : (kk >> 1) * BM * 4 + ((2 * kk) & 3) + i * 128; };
            const float *Bs = smem + stage * STAGE + BK * BM + wn0 + l31;
            if constexpr (MFK == 1) { // every fragment of the k-tile first, then the MFMAs with nothing between them
                float afa[BK / 2][TM], bfa[BK / 2][TN];
#pragma unroll
                for (int kk = 0; kk < BK / 2; kk++) {
#pragma unroll
                    for (int i = 0; i < TM; i++) afa[kk][i] = As[a_idx(kk, i)];
#pragma unroll
                    for (int j = 0; j < TN; j++) bfa[kk][j] = Bs[(2 * kk + half) * BN + j * 32];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kk = 0; kk < BK / 2; kk++)
#pragma unroll
                    for (int i = 0; i < TM; i++)
#pragma unroll
                        for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(afa[kk][i], bfa[kk][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                return;
            }
            float af[2][TM], bf[2][TN];
#pragma unroll
            for (int i = 0; i < TM; i++) af[0][i] = As[a_idx(0, i)];
#pragma unroll
            for (int j = 0; j < TN; j++) bf[0][j] = Bs[half * BN + j * 32];
#pragma unroll
            for (int kk = 0; kk < BK / 2; kk++) {
                const int cur = kk & 1, nxt = cur ^ 1;
                if (kk + 1 < BK / 2) {
#pragma unroll
                    for (int i = 0; i < TM; i++) af[nxt][i] = As[a_idx(kk + 1, i)];
#pragma unroll
                    for (int j = 0; j < TN; j++) bf[nxt][j] = Bs[(2 * (kk + 1) + half) * BN + j * 32];
                }
#pragma unroll
                for (int i = 0; i < TM; i++)
#pragma unroll
                    for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);
            }
        }
        __builtin_amdgcn_iglp_opt(0);
    };

    // fold of a finished depth block into `tot` / epilogue of a finished tile (the helpers of the one-tile kernels)
    auto flush = [&](bool first, int m0, int n0) {
        if constexpr (MF16) {
            int mb = m0 + wm0 + 4 * quad, nb0 = n0 + wn0 + l15;
            asm volatile("" : "+v"(mb), "+v"(nb0));
            if (first) fold_first16<TM2, TN2>(p, z, acc4, tot4, mb, nb0, c_zoff);
            else fold_next16<TM2, TN2>(p, acc4, tot4);
        } else {
            int mb = m0 + wm0 + 4 * half, nb0 = n0 + wn0 + l31;
            asm volatile("" : "+v"(mb), "+v"(nb0));
            if (first) fold_first<TM, TN>(p, z, acc, tot, mb, nb0, c_zoff);
            else fold_next<TM, TN>(p, acc, tot);
        }
        zero_acc();
    };
    auto finish = [&](bool single_block, int m0, int n0) {
        if constexpr (MF16) {
            int mb = m0 + wm0 + 4 * quad, nb0 = n0 + wn0 + l15;
            asm volatile("" : "+v"(mb), "+v"(nb0));
            if (single_block) {
                fold_first16<TM2, TN2>(p, z, acc4, acc4, mb, nb0, c_zoff);
                store_out16<TM2, TN2>(p, acc4, mb, nb0, c_zoff);
            } else {
                fold_next16<TM2, TN2>(p, acc4, tot4);
                store_out16<TM2, TN2>(p, tot4, mb, nb0, c_zoff);
            }
        } else {
            int mb = m0 + wm0 + 4 * half, nb0 = n0 + wn0 + l31;
            asm volatile("" : "+v"(mb), "+v"(nb0));
            if (single_block) {
                fold_first<TM, TN>(p, z, acc, acc, mb, nb0, c_zoff);
                store_out<TM, TN>(p, acc, mb, nb0, c_zoff);
            } else {
                fold_next<TM, TN>(p, acc, tot);
                store_out<TM, TN>(p, tot, mb, nb0, c_zoff);
            }
        }
        zero_acc();
    };

    // ---- the ring: NSTAGE - 1 k-tiles in flight before the first MFMA, then one barrier per k-tile for the whole list
    setup_loader(l_tile);
    fetch_lut(0);
#pragma unroll
    for (int i = 0; i < NSTAGE - 1; i++) issue_tile(i);
    zero_acc();
    int stage = 0;
    const bool single_block = nk <= KC_TILES;
#ifdef RTEN_TRACE
    unsigned long long tr_seg[5] = {0, 0, 0, 0, 0}, tr_n = 0, tr_prev = __builtin_readcyclecounter();
#define RTEN_STAMP(i) { const unsigned long long now_ = __builtin_readcyclecounter(); tr_seg[i] += now_ - tr_prev; tr_prev = now_; }
#else
#define RTEN_STAMP(i)
#endif
    for (int c_tile = t_next; c_tile < t_end; c_tile += t_step) {
        int m0, n0;
        tile_origin(c_tile, m0, n0);
        for (int kt = 0; kt < nk; kt++) {
            RTEN_STAMP(4)
            // this wave's DMA for this k-tile has landed (younger loads: one more k-tile; stores of the previous tile's epilogue
            // can only make the count conservative: loads retire in order among themselves)
            if (!(ABLATE(p) & 32)) wait_vmcnt<PER_TILE *(NSTAGE - 2)>();
            RTEN_STAMP(0)
            if (!(ABLATE(p) & 8)) __builtin_amdgcn_s_barrier(); // ... and everyone else's; all waves are done reading the stage refilled next
            RTEN_STAMP(1)
            const int stp = stage == 0 ? NSTAGE - 1 : stage - 1;
            if (!(ABLATE(p) & 1)) issue_tile(stp);
            RTEN_STAMP(2)
            if (ABLATE(p) & 16) { // ablation: the k-tile's MFMAs on register operands (no ds_read)
                if constexpr (!MF16) {
                    float fa = (float)kt, fb = (float)lane;
#pragma unroll
                    for (int kk = 0; kk < BK / 2; kk++)
#pragma unroll
                        for (int i = 0; i < TM; i++)
#pragma unroll
                            for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[i][j], 0, 0, 0);
                }
            } else if (!(ABLATE(p) & 2)) compute_tile(stage);
            RTEN_STAMP(3)
#ifdef RTEN_TRACE
            tr_n++;
#endif
            stage = stage == NSTAGE - 1 ? 0 : stage + 1;
            if (!single_block && kt + 1 < nk && (kt + 1) % KC_TILES == 0) flush(kt + 1 == KC_TILES, m0, n0);
        }
        finish(single_block, m0, n0);
    }
    wait_vmcnt<0>(); // the zero-fill look-ahead loads must land before the LDS goes away
#ifdef RTEN_TRACE
    if (blockIdx.x == 8 && blockIdx.y == 0 && lane == 0 && (wave == 0 || wave == 3))
        printf("[trace] wave %d: %llu k-tiles; cycles per k-tile: vmcnt wait %.0f, barrier %.0f, DMA issue + loader advance %.0f, fragments + MFMA issue %.0f, loop / fold / epilogue %.0f\n",
               wave, tr_n, (double)tr_seg[0] / tr_n, (double)tr_seg[1] / tr_n, (double)tr_seg[2] / tr_n, (double)tr_seg[3] / tr_n, (double)tr_seg[4] / tr_n);
#endif
#undef RTEN_STAMP
}

template <int BM, int BN, int AL, int BL>
int32_t launch(rten_hip_ctx *ctx, const GemmArgs &a, dim3 grid, int form, int dyn_lds, double flops, double bytes) {
    char kname[96];
    snprintf(kname, sizeof kname, "igemm_f32_pers_kernel<%d,%d,%d,%d,%s,%d>", BM, BN, AL, BL, form == 2 ? "true" : "false", form == 1 ? 1 : 0);
    ProfScope ps(ctx, kname, flops, bytes);
    constexpr int kStatic = 3 * BK * (BM + BN) * 4;
    auto go = [&](auto kern) {
        if (kStatic + dyn_lds > 64 * 1024) hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, dyn_lds);
        hipLaunchKernelGGL(kern, grid, dim3(NTHREADS), (size_t)dyn_lds, ctx->stream, a);
    };
    if (form == 2) go(igemm_f32_pers_kernel<BM, BN, AL, BL, true>);
    else if (form == 1) go(igemm_f32_pers_kernel<BM, BN, AL, BL, false, 1>);
    else go(igemm_f32_pers_kernel<BM, BN, AL, BL, false>);
    RTEN_LAUNCH_CHECK(ctx, "igemm_f32_pers_kernel launch");
    return RTEN_HIP_OK;
}

} // namespace

int32_t rten_launch_gemm_f32_pers(rten_hip_ctx *ctx, const void *args, unsigned grid_x, unsigned grid_z, int bm, int bn, int al, int bl, int form,
                                  int dyn_lds, double flops, double bytes) {
    const GemmArgs &a = *static_cast<const GemmArgs *>(args);
    const dim3 grid(grid_x, grid_z);
    return switch_tile(ctx, "igemm_f32_pers_kernel", bm, bn, [&](auto t) -> int32_t {
        constexpr int BM = decltype(t)::bm, BN = decltype(t)::bn;
        switch (layouts(al, bl)) {
        case layouts(A_M4, B_N4): return launch<BM, BN, A_M4, B_N4>(ctx, a, grid, form, dyn_lds, flops, bytes);
        case layouts(A_M4, B_IM2COL): return launch<BM, BN, A_M4, B_IM2COL>(ctx, a, grid, form, dyn_lds, flops, bytes);
        case layouts(A_M4, B_IM2COL_TAPS): return launch<BM, BN, A_M4, B_IM2COL_TAPS>(ctx, a, grid, form, dyn_lds, flops, bytes);
        case layouts(A_K4, B_N4): return launch<BM, BN, A_K4, B_N4>(ctx, a, grid, form, dyn_lds, flops, bytes);
        default: return not_covered(ctx, "igemm_f32_pers_kernel");
        }
    });
}
