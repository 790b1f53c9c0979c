// The LDS-DMA family of the f32 implicit-GEMM kernels (gfx950): igemm_f32_dma_kernel in its two- / three- / four-stage, fragments-first and
// mixed (whole tiles + split-K producers in one launch) forms, and the split-K fixup kernel.  Launch plans: gemm_f32.hip.
#include "gemm_f32_common.h"

namespace {

// =====================================================================================================
// LDS-DMA variant (conv paths: A = prepacked [K][M] weights, B = dense two-level or im2col gather).
//
// Tiles go HBM/L2 -> LDS directly (`buffer_load_dword[x4] ... offen lds`): no staging VGPRs, no ds_write
// pass, and three LDS stages keep two k-tiles in flight behind the one being multiplied, so the
// ~1200-cycle load latency hides under the matrix pipe even when only one or two workgroups fit on a CU.
// Per k-tile: counted `s_waitcnt vmcnt(N)` (never 0 inside the loop) -> raw s_barrier -> issue the DMA of
// tile kt+2 into the stage that was just freed -> MFMAs of tile kt (operand fragments double buffered in
// registers so ds_read latency overlaps the previous MFMA group).  All LDS lives in ONE __shared__
// array (a second object would make hipcc drain vmcnt before every ds_read -- cdna_hip_programming.md).
// LDS image: As[BK][BM], Bs[BK][BN] unpadded (DMA writes are lane-linear); MFMA operand reads walk
// consecutive columns, so they are conflict-free without padding.
// =====================================================================================================
// MODE 0: K <= 256 (one depth block); 1: several depth blocks folded in registers; 2: split-K producer -- every
// workgroup computes one group of depth blocks of one split tile and parks each block's raw accumulator in the slab
// (no fold, no epilogue: igemm_f32_fixup_kernel finishes the tile).
// AL: A_M4 = k-major A ([K][M], prepacked conv weights, transposed GEMM operands); A_K4 = row-major A ([M][K], the
// plain MatMul layout): one DMA instruction then moves 64 rows x one k-quad and the LDS image is [k-quad][m][4].
// MFK: 0 = operand fragments double buffered across k-pairs with the next pair's ds_reads behind the current MFMA group (iglp_opt);
//      1 = all of the k-tile's fragments first, then the MFMAs back to back with nothing between them: with one 32x32 block per
//          wave (64x64 tiles) consecutive MFMAs hit the SAME accumulator, and any instruction issued between two such MFMAs
//          costs ~43 cycles on top of its own slot (MI355X_MICROARCH.md, per-instruction constants).
// Waves per SIMD the compiler must leave room for: 64x64 tiles are LDS-limited to 6 (three stages) / 10 (two stages) workgroups per compute unit,
// so their register budget is set to match (80 VGPRs: the MODE 1 / 2 forms sat at 81-85, i.e. at 5) -- more resident workgroups is what these
// kernels respond to (tools/debug/f32_trace.py with RTEN_HIP_OCC_CAP: 2 -> 3 -> 6 workgroups per CU = 3.72 -> 3.20 -> 2.95 ms per step).
// (four stages of a 64x64 tile are 32 KB: LDS admits four to five workgroups per compute unit, so asking the compiler for a six-wave register budget only made it
// report an unmet target -- rounds 3-5; the four-stage forms now ask for what they can have)
constexpr int dma_min_waves(int bm, int bn, int mode, int nst = 3) { return bm * bn == 64 * 64 ? ((mode == 3 || nst >= 4) ? 4 : 6) : 2; }
template <int BM, int BN, int AL, int BL, int MODE, int NST = 3, int MFK = 0>
__global__ __launch_bounds__(NTHREADS, dma_min_waves(BM, BN, MODE, NST)) void igemm_f32_dma_kernel(const GemmArgs p) {
    TR_DECL
    TR_STAMP(0)
    kernarg_prefetch<(int)sizeof(GemmArgs)>();
    // MODE 3 ("mixed"): one launch holds the whole tiles [0, split_t1) (fold + epilogue, as MODE 1) AND the split-K
    // producers of the tail tiles (as MODE 2), so the tail's small workgroups fill the last round next to the whole
    // tiles instead of running alone afterwards.
    constexpr bool MIXED = MODE == 3, MULTI_KC = MODE == 1 || MIXED, SPLIT = MODE == 2;
    static_assert(AL == A_M4 || AL == A_K4, "DMA kernel: A is k-major or row-major with 16-byte rows");
    static_assert(BL == B_N4 || BL == B_IM2COL || BL == B_IM2COL_TAPS, "DMA kernel covers the conv operand layouts");
    constexpr int WM = 2, WN = 2;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int STAGE = BK * (BM + BN); // floats per stage
    constexpr int NA = BK * BM / 256 / 4; // dwordx4 DMA instructions per wave per tile (A)
    constexpr int NBV = BK * BN / 256 / 4; // dwordx4 (dense B)
    constexpr int NBG = BK * BN / 64 / 4;  // dword gathers per wave per tile (im2col B)
    constexpr int PER_TILE = NA + (BL == B_N4 ? NBV : NBG);
    static_assert(NA >= 1 && NBV >= 1, "tile too small for 4-wave DMA split");
    constexpr int NSTAGE = NST;
    __shared__ __attribute__((aligned(16))) float smem[NSTAGE * STAGE];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int z = blockIdx.y;

    int tile, grp = -1; // grp >= 0: this workgroup computes one K group of a split tile
    {
        const int id = blockIdx.x;
        const int nt = MIXED ? p.split_t1 : (int)gridDim.x; // whole tiles are XCD-chunked; mixed-mode producers keep dispatch order
        tile = xcd_chunked_tile(id, nt);
        if (SPLIT || (MIXED && id >= p.split_t1)) {
            const int rr = MIXED ? id - p.split_t1 : tile;
            if (p.order & 2) { // K group slowest: an XCD's contiguous id range is one K slice of many tiles
                grp = rr / p.split_ntail;
                tile = p.split_t1 + rr - grp * p.split_ntail;
            } else {           // K group fastest: an XCD's range is all K slices of a few tiles
                tile = p.split_t1 + rr / p.split_s;
                grp = rr - (rr / p.split_s) * p.split_s;
            }
        }
    }
    const int bm = (p.order & 1) ? tile / p.tiles_n : tile % p.tiles_m, bn = (p.order & 1) ? tile % p.tiles_n : tile / p.tiles_m;
    const int m0 = bm * BM, n0 = bn * BN;

    const BatchSlice zs = batch_slice(p, z);
    const long long c_zoff = zs.c_zoff;
    const __amdgpu_buffer_rsrc_t rsA = slice_rsrc(zs.A, p.a_bytes), rsB = slice_rsrc(zs.B, p.b_bytes);
    const int nk = (p.K + BK - 1) / BK;

    // ---- loop-invariant DMA source offsets.  Wave w issues instructions q = w*N + j; instruction q covers
    // the flat tile range [q*256, q*256+256) floats (dwordx4) or [q*64, q*64+64) (dword gather).
    unsigned a_voff[NA];
    [[maybe_unused]] int a_kq[NA]; // A_K4: first local k of the instruction's k-quad (k-tail test)
    dma_a_offsets<BM, AL, NA>(p, m0, wave, lane, a_voff, a_kq);
    const unsigned a_kstep = AL == A_M4 ? (unsigned)(BK * p.a_cs * 4) : (unsigned)(BK * 4);

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
        for (int j = 0; j < NA; j++) {
            bool dead = past;
            if constexpr (AL == A_K4) dead = a_kq[j] >= p.K - kt * BK; // k-tail quads (and every quad past the end) read as zeros
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_t)(As + (wave * NA + j) * 256), 16,
                                                     (int)(dead ? OOB : a_voff[j]), (int)a_soff, 0, 0);
        }
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
    const int wq = t >> 6; // per-lane copy of the wave id for address math
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
        // A fragment of k-pair kk, block i: k = 2*kk + half.  k-major image: As[k][m]; row-major image: [k/4][m][4]
        // (k and k+1 share a quad, so `half` is part of the lane's base and the rest is an immediate).
        const float *As = smem + stage * STAGE + (AL == A_M4 ? wm0 + l31 + half * BM : (wm0 + l31) * 4 + half);
        auto a_idx = [](int kk, int i) { return AL == A_M4 ? 2 * kk * BM + i * 32 : (kk >> 1) * BM * 4 + ((2 * kk) & 3) + i * 128; };
        const float *Bs = smem + stage * STAGE + BK * BM + wn0 + l31;
        if constexpr (MFK == 1) {
            float afa[BK / 2][TM], bfa[BK / 2][TN];
#pragma unroll
            for (int kk = 0; kk < BK / 2; kk++) {
#pragma unroll
                for (int i = 0; i < TM; i++) afa[kk][i] = As[a_idx(kk, i)];
#pragma unroll
                for (int j = 0; j < TN; j++) bfa[kk][j] = Bs[(2 * kk + half) * BN + j * 32];
            }
            __builtin_amdgcn_sched_barrier(0); // every ds_read of the tile is issued before the first MFMA
#pragma unroll
            for (int kk = 0; kk < BK / 2; kk++)
#pragma unroll
                for (int i = 0; i < TM; i++)
#pragma unroll
                    for (int j = 0; j < TN; j++)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(afa[kk][i], bfa[kk][j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            return;
        }
        float af[2][TM], bf[2][TN]; // operand fragments, double buffered across k-pairs
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
                for (int j = 0; j < TN; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_iglp_opt(0);
    };

    [[maybe_unused]] auto store_raw = [&](f32x16 (&v)[TM][TN], int slot) { split_park<BM, BN, TM, TN>(p, z, tile, wq, lane, v, slot); };

    // ---- software pipeline: tiles kt+1 and kt+2 are in flight while tile kt is multiplied
    const int nblk = (MULTI_KC || SPLIT) ? (nk + KC_TILES - 1) / KC_TILES : 1;
    int blk0 = 0, blk1 = nblk;
    if (SPLIT || (MIXED && grp >= 0)) {
        blk0 = grp * p.split_g;
        blk1 = blk0 + p.split_g < nblk ? blk0 + p.split_g : nblk;
    }
    const int kt0 = blk0 * KC_TILES;
    fetch_lut(kt0);
#pragma unroll
    for (int i = 0; i < NSTAGE - 1; i++) {
        issue_tile(kt0 + i, i);
        fetch_lut(kt0 + i + 1);
    }
    int stage = 0;
    TR_STAMP(1)
    for (int blk = blk0; blk < blk1; blk++) {
        const int kt_end = (MULTI_KC || SPLIT) ? ((blk + 1) * KC_TILES < nk ? (blk + 1) * KC_TILES : nk) : nk;
        for (int kt = blk * KC_TILES; kt < kt_end; kt++) {
            wait_vmcnt<PER_TILE *(NSTAGE - 2)>(); // this wave's DMA for tile kt has landed; NSTAGE-2 later tiles stay in flight
            if (!(ABLATE(p) & 8)) __builtin_amdgcn_s_barrier(); // ... and everyone else's; all waves are done reading the stage of tile kt-1
#ifdef RTEN_TRACE
            if (tr_trips == 0) TR_STAMP(2)
            tr_trips++;
#endif
            const int stp = stage == 0 ? NSTAGE - 1 : stage - 1; // (kt + NSTAGE - 1) % NSTAGE: the stage tile kt-1 used
            if (!(ABLATE(p) & 1)) issue_tile(kt + NSTAGE - 1, stp);
            fetch_lut(kt + NSTAGE);
            if (ABLATE(p) & 16) { // ablation: MFMAs on register operands only (no ds_read)
                float fa = (float)kt, fb = (float)lane;
#pragma unroll
                for (int kk = 0; kk < BK / 2; kk++)
#pragma unroll
                    for (int i = 0; i < TM; i++)
#pragma unroll
                        for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[i][j], 0, 0, 0);
            } else if (!(ABLATE(p) & 2)) compute_tile(stage); // (s_setprio around the matrix phase: measured, no gain)
            stage = stage == NSTAGE - 1 ? 0 : stage + 1;
        }
        if (SPLIT || (MIXED && grp >= 0)) {
            // order bit 3 (RELAXED split-K, measurement only, NOT the reference's order): the group's depth blocks accumulate in one register block and ONE
            // partial per group is parked (slot = group) -- what an order-free split-K would move; the strict form parks every depth block
            const bool relaxed = (p.order & 8) != 0;
            if (!relaxed || blk + 1 == blk1) {
                store_raw(acc, relaxed ? grp : blk);
#pragma unroll
                for (int i = 0; i < TM; i++)
#pragma unroll
                    for (int j = 0; j < TN; j++)
#pragma unroll
                        for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
            }
        } else if constexpr (MULTI_KC) {
            if (blk + 1 < nblk) flush(blk == 0);
        }
    }
    wait_vmcnt<0>(); // drain the two look-ahead tiles before the LDS goes away
    TR_STAMP(3)
    [[maybe_unused]] constexpr unsigned TR_KID = BM | (BN << 8) | (MODE << 16) | (BL << 20) | (AL << 24) | (NST << 28);

    if (SPLIT || (MIXED && grp >= 0)) {
        if (p.split_counters) split_finish<BM, BN, TM, TN>(p, z, tile, wq, lane, m0, n0, c_zoff, reinterpret_cast<int *>(smem));
        TR_STAMP(4)
        TR_WRITE(TR_KID, tile, grp)
        return;
    }
    if constexpr (!SPLIT) {
        if (!(ABLATE(p) & 4)) {
            const int mb = m0 + wm0 + 4 * half, nb0 = n0 + wn0 + l31;
            if constexpr (MULTI_KC) { // launched only for K > 256: at least two depth blocks
                fold_next<TM, TN>(p, acc, tot);
                store_out<TM, TN>(p, tot, mb, nb0, c_zoff);
            } else {
                fold_first<TM, TN>(p, z, acc, acc, mb, nb0, c_zoff);
                store_out<TM, TN>(p, acc, mb, nb0, c_zoff);
            }
        }
    }
    TR_STAMP(4)
    TR_WRITE(TR_KID, tile, grp)
}

// Split-K fixup: one WAVE per quadrant of a split tile (grid = 4 x split tiles, 64 threads), same lane <-> element
// mapping as the GEMM kernels.  Replays the unsplit kernel's fold over the parked per-block accumulators in
// depth-block order (first block: beta*C + bias; later blocks: separate adds), then the shared epilogue (residual,
// activation, store).  Slots are fetched U at a time so several loads are in flight per lane.
template <int BM, int BN>
__global__ __launch_bounds__(64) void igemm_f32_fixup_kernel(const GemmArgs p) {
    kernarg_prefetch<(int)sizeof(GemmArgs)>();
    constexpr int WM = 2, WN = 2;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int U = TM * TN >= 4 ? 1 : 4 / (TM * TN); // slots per batch: 64 floats per lane in flight
    const int lane = threadIdx.x, wq = blockIdx.x & 3, ti = blockIdx.x >> 2;
    const int l31 = lane & 31, half = lane >> 5;
    const int z = blockIdx.y;
    const int tile = p.split_t1 + ti;
    const int bm = (p.order & 1) ? tile / p.tiles_n : tile % p.tiles_m, bn = (p.order & 1) ? tile % p.tiles_n : tile / p.tiles_m;
    const int m0 = bm * BM, n0 = bn * BN;
    const long long c_zoff = batch_slice(p, z).c_zoff;
    const int wm0 = (wq / WN) * (BM / WM), wn0 = (wq % WN) * (BN / WN);
    const float *base = p.slab + ((long long)z * p.split_ntail + ti) * p.split_slots * (long long)(BM * BN) +
                        wq * (TM * TN * 16 * 64) + lane * 4;
    f32x16 acc[U][TM][TN], tot[TM][TN];
    auto load_raw = [&](f32x16 (&v)[TM][TN], int slot) {
        const float *b = base + (long long)slot * (BM * BN);
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const f32x4 o = *(const f32x4 *)(b + ((i * TN + j) * 4 + q) * 256);
                    v[i][j][4 * q] = o[0]; v[i][j][4 * q + 1] = o[1]; v[i][j][4 * q + 2] = o[2]; v[i][j][4 * q + 3] = o[3];
                }
    };
    const int mb = m0 + wm0 + 4 * half, nb0 = n0 + wn0 + l31;
    load_raw(acc[0], 0);
    fold_first<TM, TN>(p, z, acc[0], tot, mb, nb0, c_zoff);
    int s = 1;
    for (; s + U <= p.split_slots; s += U) {
#pragma unroll
        for (int u = 0; u < U; u++) load_raw(acc[u], s + u);
#pragma unroll
        for (int u = 0; u < U; u++) fold_next<TM, TN>(p, acc[u], tot);
    }
    for (; s < p.split_slots; s++) {
        load_raw(acc[0], s);
        fold_next<TM, TN>(p, acc[0], tot);
    }
    store_out<TM, TN>(p, tot, mb, nb0, c_zoff);
}

// One (stage count, MFMA issue form): MODE 0 / 1 / 2 onto the template parameter, launch, check.
template <int BM, int BN, int AL, int BL, int NST, int MFK>
int32_t launch_modes(rten_hip_ctx *ctx, const GemmArgs &a, dim3 grid, int mode, size_t dyn_lds) {
    if (mode == 2) hipLaunchKernelGGL((igemm_f32_dma_kernel<BM, BN, AL, BL, 2, NST, MFK>), grid, dim3(NTHREADS), dyn_lds, ctx->stream, a);
    else if (mode == 1) hipLaunchKernelGGL((igemm_f32_dma_kernel<BM, BN, AL, BL, 1, NST, MFK>), grid, dim3(NTHREADS), dyn_lds, ctx->stream, a);
    else hipLaunchKernelGGL((igemm_f32_dma_kernel<BM, BN, AL, BL, 0, NST, MFK>), grid, dim3(NTHREADS), dyn_lds, ctx->stream, a);
    RTEN_LAUNCH_CHECK(ctx, "igemm_f32_dma_kernel launch");
    return RTEN_HIP_OK;
}

// mode 3 = mixed (three stages only, tiles below 128x128); nst = 2 exists for 64x64 tiles; mfk = 1 with three stages
template <int BM, int BN, int AL, int BL>
int32_t launch(rten_hip_ctx *ctx, const GemmArgs &a, dim3 grid, int mode, int nst, int mfk, size_t dyn_lds, double flops, double bytes) {
    char kname[96];
    if (mode == 3) {
        if constexpr (BM * BN < 128 * 128) {
            snprintf(kname, sizeof kname, "igemm_f32_dma_kernel<%d,%d,%d,%d,3,3>", BM, BN, AL, BL);
            ProfScope ps(ctx, kname, flops, bytes);
            hipLaunchKernelGGL((igemm_f32_dma_kernel<BM, BN, AL, BL, 3>), grid, dim3(NTHREADS), dyn_lds, ctx->stream, a);
            RTEN_LAUNCH_CHECK(ctx, "igemm_f32_dma_kernel (mixed) launch");
            return RTEN_HIP_OK;
        }
        return not_covered(ctx, "igemm_f32_dma_kernel (mixed)");
    }
    if (mfk) snprintf(kname, sizeof kname, "igemm_f32_dma_kernel<%d,%d,%d,%d,%d,3,1>", BM, BN, AL, BL, mode);
    else snprintf(kname, sizeof kname, "igemm_f32_dma_kernel<%d,%d,%d,%d,%d,%d>", BM, BN, AL, BL, mode, nst);
    ProfScope ps(ctx, kname, flops, bytes);
    if (mfk) return launch_modes<BM, BN, AL, BL, 3, 1>(ctx, a, grid, mode, dyn_lds);
    if (nst == 4) return launch_modes<BM, BN, AL, BL, 4, 0>(ctx, a, grid, mode, dyn_lds);
    if constexpr (BM == 64 && BN == 64) {
        if (nst == 2) return launch_modes<BM, BN, AL, BL, 2, 0>(ctx, a, grid, mode, dyn_lds);
    }
    if (nst == 3) return launch_modes<BM, BN, AL, BL, 3, 0>(ctx, a, grid, mode, dyn_lds);
    return not_covered(ctx, "igemm_f32_dma_kernel");
}

template <int BM, int BN>
int32_t launch_fixup(rten_hip_ctx *ctx, const GemmArgs &a, dim3 grid, double bytes) {
    char kname[96];
    snprintf(kname, sizeof kname, "igemm_f32_fixup_kernel<%d,%d>", BM, BN);
    ProfScope ps(ctx, kname, 0.0, bytes);
    hipLaunchKernelGGL((igemm_f32_fixup_kernel<BM, BN>), grid, dim3(64), 0, ctx->stream, a);
    RTEN_LAUNCH_CHECK(ctx, "igemm_f32_fixup_kernel launch");
    return RTEN_HIP_OK;
}

} // namespace

int32_t rten_launch_gemm_f32_dma(rten_hip_ctx *ctx, const void *args, unsigned grid_x, unsigned grid_z, int bm, int bn, int al, int bl, int mode, int nst,
                                 int mfk, size_t dyn_lds, double flops, double bytes) {
    TRACED_ARGS(a, args, grid_x * grid_z);
    const dim3 grid(grid_x, grid_z);
    return switch_tile(ctx, "igemm_f32_dma_kernel", bm, bn, [&](auto t) -> int32_t {
        constexpr int BM = decltype(t)::bm, BN = decltype(t)::bn;
        switch (layouts(al, bl)) {
        case layouts(A_M4, B_N4): return launch<BM, BN, A_M4, B_N4>(ctx, a, grid, mode, nst, mfk, dyn_lds, flops, bytes);
        case layouts(A_M4, B_IM2COL): return launch<BM, BN, A_M4, B_IM2COL>(ctx, a, grid, mode, nst, mfk, dyn_lds, flops, bytes);
        case layouts(A_M4, B_IM2COL_TAPS): return launch<BM, BN, A_M4, B_IM2COL_TAPS>(ctx, a, grid, mode, nst, mfk, dyn_lds, flops, bytes);
        case layouts(A_K4, B_N4): return launch<BM, BN, A_K4, B_N4>(ctx, a, grid, mode, nst, mfk, dyn_lds, flops, bytes);
        default: return not_covered(ctx, "igemm_f32_dma_kernel");
        }
    });
}

int32_t rten_launch_gemm_f32_fixup(rten_hip_ctx *ctx, const void *args, unsigned grid_x, unsigned grid_z, int bm, int bn, double bytes) {
    const GemmArgs &a = *static_cast<const GemmArgs *>(args);
    return switch_tile(ctx, "igemm_f32_fixup_kernel", bm, bn, [&](auto t) -> int32_t {
        return launch_fixup<decltype(t)::bm, decltype(t)::bn>(ctx, a, dim3(grid_x, grid_z), bytes);
    });
}
