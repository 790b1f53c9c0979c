// The register-staged family of the f32 GEMM / implicit-GEMM kernels (gfx950): tiles go global -> VGPRs -> LDS, double buffered.  It takes
// every operand layout the planner of gemm_f32.hip knows except the tap-masked im2col gather -- the plain MatMul layouts and the scalar
// loaders run nowhere else (pipeline 0; GEMM variants 4..7 on the conv layouts).  The mapping onto the MI355X is described in gemm_f32.hip.
#include "gemm_f32_common.h"

namespace {

// MODE: 0 = one depth block, 1 = several depth blocks folded in registers, 2 = split-K producer (see the LDS-DMA kernel).
template <int BM, int BN, int AL, int BL, int MODE>
__global__ __launch_bounds__(NTHREADS, 2) void igemm_f32_kernel(const GemmArgs p) {
    kernarg_prefetch<(int)sizeof(GemmArgs)>();
    constexpr bool MULTI_KC = MODE == 1, SPLIT = MODE == 2;
    constexpr int WM = 2, WN = 2;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int A_ELEMS = BK * BM / NTHREADS, B_ELEMS = BK * BN / NTHREADS; // per-thread elements per tile
    constexpr int NA = (AL == A_SCALAR) ? A_ELEMS : A_ELEMS / 4;              // loads per thread per tile
    constexpr int NB = (BL == B_SCALAR || BL == B_IM2COL) ? B_ELEMS : B_ELEMS / 4;
    static_assert((NTHREADS / BN) * B_ELEMS == BK, "im2col row mapping must cover the k-tile");
    __shared__ __attribute__((aligned(16))) float smem[2 * BK * (LDA + LDB)];
    float *const As0 = smem;
    float *const Bs0 = smem + 2 * BK * LDA;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int z = blockIdx.y;

    // ---- XCD-aware tile mapping: consecutive ids on one XCD walk down a column of tiles (same B panel)
    int tile, grp = -1; // grp >= 0: this workgroup computes one K group of a split tile
    {
        tile = xcd_chunked_tile(blockIdx.x, gridDim.x);
        if constexpr (SPLIT) {
            const int rr = tile;
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

    // ---- per-thread, loop-invariant byte offsets.  OOB marks lanes outside the tile's valid rows/columns.
    unsigned a_voff[NA];
    int a_krow[NA]; // local k of the element (k-tail test)
    unsigned a_kstep; // byte advance per k-tile (soffset)
    if constexpr (AL == A_M4) { // float4 along m, rows of the K x M (prepacked / transposed) operand
#pragma unroll
        for (int j = 0; j < NA; j++) {
            const int idx = t + j * NTHREADS;
            const int k = idx / (BM / 4), m = m0 + (idx % (BM / 4)) * 4;
            a_krow[j] = k;
            a_voff[j] = m < p.M ? (unsigned)(((long long)k * p.a_cs + m) * 4) : OOB;
        }
        a_kstep = (unsigned)(BK * p.a_cs * 4);
    } else if constexpr (AL == A_K4) { // float4 along k of a row-major [M][K] operand
#pragma unroll
        for (int j = 0; j < NA; j++) {
            const int idx = t + j * NTHREADS;
            const int k = (idx % (BK / 4)) * 4, m = m0 + idx / (BK / 4);
            a_krow[j] = k;
            a_voff[j] = m < p.M ? (unsigned)(((long long)m * p.a_rs + k) * 4) : OOB;
        }
        a_kstep = BK * 4;
    } else {
#pragma unroll
        for (int j = 0; j < NA; j++) {
            const int idx = t + j * NTHREADS;
            const int k = p.a_dir_m ? idx / BM : idx % BK;
            const int m = m0 + (p.a_dir_m ? idx % BM : idx / BK);
            a_krow[j] = k;
            a_voff[j] = m < p.M ? (unsigned)(((long long)m * p.a_rs + (long long)k * p.a_cs) * 4) : OOB;
        }
        a_kstep = (unsigned)(BK * p.a_cs * 4);
    }

    [[maybe_unused]] unsigned b_voff[NB];
    [[maybe_unused]] int b_krow[NB];
    [[maybe_unused]] unsigned b_kstep = 0;
    [[maybe_unused]] int im_iy0 = 0, im_ix0 = 0, im_pix = 0;
    if constexpr (BL == B_N4) {
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int idx = t + j * NTHREADS;
            const int k = idx / (BN / 4), n = n0 + (idx % (BN / 4)) * 4;
            const int nn = n < p.N ? n : 0;
            const int nb = nn / p.Pn, np = nn - nb * p.Pn;
            b_krow[j] = k;
            b_voff[j] = n < p.N ? (unsigned)(((long long)k * p.b_rs + (long long)nb * p.b_ns + np) * 4) : OOB;
        }
        b_kstep = (unsigned)(BK * p.b_rs * 4);
    } else if constexpr (BL == B_K4) {
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int idx = t + j * NTHREADS;
            const int k = (idx % (BK / 4)) * 4, n = n0 + idx / (BK / 4);
            const int nn = n < p.N ? n : 0;
            const int nb = nn / p.Pn, np = nn - nb * p.Pn;
            b_krow[j] = k;
            b_voff[j] = n < p.N ? (unsigned)(((long long)nb * p.b_ns + (long long)np * p.b_cs + k) * 4) : OOB;
        }
        b_kstep = BK * 4;
    } else if constexpr (BL == B_SCALAR) {
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int idx = t + j * NTHREADS;
            const int k = p.b_dir_n ? idx / BN : idx % BK;
            const int n = n0 + (p.b_dir_n ? idx % BN : idx / BK);
            const int nn = n < p.N ? n : 0;
            const int nb = nn / p.Pn, np = nn - nb * p.Pn;
            b_krow[j] = k;
            b_voff[j] = n < p.N ? (unsigned)(((long long)k * p.b_rs + (long long)nb * p.b_ns + (long long)np * p.b_cs) * 4) : OOB;
        }
        b_kstep = (unsigned)(BK * p.b_rs * 4);
    } else { // B_IM2COL: thread owns column t % BN and rows (t / BN) * B_ELEMS + j (consecutive -> contiguous LUT reads)
        const int n = n0 + (t % BN);
        const bool ok = n < p.N;
        const int nn = ok ? n : 0;
        const int nb = nn / p.Pn, np = nn - nb * p.Pn;
        const int oy = np / p.OW, ox = np - oy * p.OW;
        im_iy0 = oy * p.sy - p.pt;
        im_ix0 = ox * p.sx - p.pl;
        im_pix = (int)((long long)nb * p.b_ns) + im_iy0 * p.W + im_ix0; // element offset of the (ky=0,kx=0) tap; may be < 0
        if (!ok) im_iy0 = -0x40000000;                                  // fails every bounds test
    }

    float ra[A_ELEMS], rb[B_ELEMS];
    const int nk = (p.K + BK - 1) / BK;

    // im2col LUT entries of the tile that will be prefetched next; read with scalar loads (constant address
    // space + wave-uniform row) one iteration before they are needed, so the gather never waits on them
    typedef const __attribute__((address_space(4))) i32x2 *lut_ptr_t;
    [[maybe_unused]] i32x2 lutE[B_ELEMS];
    [[maybe_unused]] auto fetch_lut = [&](int kt) {
        if constexpr (BL == B_IM2COL) {
            int krow0 = kt * BK + (t / BN) * B_ELEMS;
            if constexpr (BN >= 64) krow0 = __builtin_amdgcn_readfirstlane(krow0);
            const lut_ptr_t lc = (lut_ptr_t)(unsigned long long)p.lut;
#pragma unroll
            for (int j = 0; j < B_ELEMS; j++) lutE[j] = lc[krow0 + j];
        }
    };

    // ---- global -> register prefetch of k-tile kt (no branches; invalid lanes read 0 through the OOB offset)
    auto load_tile = [&](int kt) {
        const int k0 = kt * BK;
        // the scalar offset never leaves the buffer (the range check subtracts it from num_records): the
        // past-the-end prefetch reuses the last tile's soffset with every lane's voffset out of range
        const int kts = kt < nk ? kt : (nk > 0 ? nk - 1 : 0);
        const unsigned a_soff = (unsigned)kts * a_kstep;
        const int kleft = p.K - k0; // rows >= kleft are the k tail
        if constexpr (AL == A_SCALAR) {
#pragma unroll
            for (int j = 0; j < NA; j++) ra[j] = buf_load1(rsA, a_krow[j] < kleft ? a_voff[j] : OOB, a_soff);
        } else {
#pragma unroll
            for (int j = 0; j < NA; j++) {
                const f32x4 v = buf_load4(rsA, a_krow[j] < kleft ? a_voff[j] : OOB, a_soff);
                ra[4 * j + 0] = v[0]; ra[4 * j + 1] = v[1]; ra[4 * j + 2] = v[2]; ra[4 * j + 3] = v[3];
            }
        }
        if constexpr (BL == B_IM2COL) {
            // virtual im2col row k -> (c, ky, kx) from the LUT entries fetched one iteration ahead
            // (rten-gemm/src/im2col.rs:145-208: out-of-image -> 0)
#pragma unroll
            for (int j = 0; j < B_ELEMS; j++) {
                const i32x2 e = lutE[j];
                const int iy = im_iy0 + (e[1] & 0xffff);
                const int ix = im_ix0 + (e[1] >> 16);
                const bool ok = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                rb[j] = buf_load1(rsB, ok ? (unsigned)(im_pix + e[0]) << 2 : OOB, 0);
            }
        } else if constexpr (BL == B_SCALAR) {
            const unsigned b_soff = (unsigned)kts * b_kstep;
#pragma unroll
            for (int j = 0; j < NB; j++) rb[j] = buf_load1(rsB, b_krow[j] < kleft ? b_voff[j] : OOB, b_soff);
        } else {
            const unsigned b_soff = (unsigned)kts * b_kstep;
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const f32x4 v = buf_load4(rsB, b_krow[j] < kleft ? b_voff[j] : OOB, b_soff);
                rb[4 * j + 0] = v[0]; rb[4 * j + 1] = v[1]; rb[4 * j + 2] = v[2]; rb[4 * j + 3] = v[3];
            }
        }
    };

    auto store_tile = [&](int buf) {
        float *As = As0 + buf * BK * LDA;
        float *Bs = Bs0 + buf * BK * LDB;
        if constexpr (AL == A_M4) {
#pragma unroll
            for (int j = 0; j < NA; j++) {
                const int idx = t + j * NTHREADS;
                const f32x4 v = {ra[4 * j], ra[4 * j + 1], ra[4 * j + 2], ra[4 * j + 3]};
                *reinterpret_cast<f32x4 *>(As + (idx / (BM / 4)) * LDA + (idx % (BM / 4)) * 4) = v;
            }
        } else if constexpr (AL == A_K4) {
#pragma unroll
            for (int j = 0; j < NA; j++) {
                const int idx = t + j * NTHREADS;
                const int k = (idx % (BK / 4)) * 4, m = idx / (BK / 4);
#pragma unroll
                for (int i = 0; i < 4; i++) As[(k + i) * LDA + m] = ra[4 * j + i];
            }
        } else {
#pragma unroll
            for (int j = 0; j < NA; j++) {
                const int idx = t + j * NTHREADS;
                As[(p.a_dir_m ? idx / BM : idx % BK) * LDA + (p.a_dir_m ? idx % BM : idx / BK)] = ra[j];
            }
        }
        if constexpr (BL == B_N4) {
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const int idx = t + j * NTHREADS;
                const f32x4 v = {rb[4 * j], rb[4 * j + 1], rb[4 * j + 2], rb[4 * j + 3]};
                *reinterpret_cast<f32x4 *>(Bs + (idx / (BN / 4)) * LDB + (idx % (BN / 4)) * 4) = v;
            }
        } else if constexpr (BL == B_K4) {
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const int idx = t + j * NTHREADS;
                const int k = (idx % (BK / 4)) * 4, n = idx / (BK / 4);
#pragma unroll
                for (int i = 0; i < 4; i++) Bs[(k + i) * LDB + n] = rb[4 * j + i];
            }
        } else if constexpr (BL == B_SCALAR) {
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const int idx = t + j * NTHREADS;
                Bs[(p.b_dir_n ? idx / BN : idx % BK) * LDB + (p.b_dir_n ? idx % BN : idx / BK)] = rb[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < B_ELEMS; j++) Bs[((t / BN) * B_ELEMS + j) * LDB + (t % BN)] = rb[j];
        }
    };

    // ---- accumulators
    const int wm0 = (wave / WN) * (BM / WM), wn0 = (wave % WN) * (BN / WN);
    f32x16 acc[TM][TN];
    [[maybe_unused]] f32x16 tot[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    // flush of one finished depth block into `tot` (between depth blocks, MULTI_KC only)
    // The row/column bases are laundered through an empty asm so that the (rare) flush's address
    // arithmetic is recomputed here instead of being hoisted out of the K loop (~100 live VGPRs).
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

    auto compute_tile = [&](int cur) {
        const float *As = As0 + cur * BK * LDA + wm0 + l31;
        const float *Bs = Bs0 + cur * BK * LDB + wn0 + l31;
        // all MFMA operands of the tile first (ds_read latency overlaps), then the MFMAs back to back
        float af[BK / 2][TM], bf[BK / 2][TN];
#pragma unroll
        for (int kk = 0; kk < BK / 2; kk++) {
#pragma unroll
            for (int i = 0; i < TM; i++) af[kk][i] = As[(2 * kk + half) * LDA + i * 32];
#pragma unroll
            for (int j = 0; j < TN; j++) bf[kk][j] = Bs[(2 * kk + half) * LDB + j * 32];
        }
#pragma unroll
        for (int kk = 0; kk < BK / 2; kk++)
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < TN; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk][i], bf[kk][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_iglp_opt(0);
    };

    [[maybe_unused]] auto store_raw = [&](f32x16 (&v)[TM][TN], int slot) { split_park<BM, BN, TM, TN>(p, z, tile, wave, lane, v, slot); };

    // ---- main loop: depth blocks of KC_TILES k-tiles; inside a block the loop body is branch free
    const int nblk = (MULTI_KC || SPLIT) ? (nk + KC_TILES - 1) / KC_TILES : 1;
    int blk0 = 0, blk1 = nblk;
    if constexpr (SPLIT) {
        blk0 = grp * p.split_g;
        blk1 = blk0 + p.split_g < nblk ? blk0 + p.split_g : nblk;
    }
    const int kt0 = blk0 * KC_TILES; // even: the double-buffer parity of tile kt stays kt & 1
    fetch_lut(kt0);
    load_tile(kt0);
    fetch_lut(kt0 + 1);
    store_tile(0);
    __syncthreads();
    for (int blk = blk0; blk < blk1; blk++) {
        const int kt_end = (MULTI_KC || SPLIT) ? ((blk + 1) * KC_TILES < nk ? (blk + 1) * KC_TILES : nk) : nk;
        for (int kt = blk * KC_TILES; kt < kt_end; kt++) {
            load_tile(kt + 1); // prefetch; past the end every lane is out of range -> zeros, never used
            fetch_lut(kt + 2);
            compute_tile(kt & 1);
            store_tile((kt + 1) & 1);
            __syncthreads();
        }
        if constexpr (SPLIT) {
            store_raw(acc, blk);
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < TN; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
        }
        if constexpr (MULTI_KC) {
            if (blk + 1 < nblk) flush(blk == 0);
        }
    }

    // ---- final depth block + fused epilogue (residual Add, activation), NCHW / row-major store
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
    } else if (p.split_counters) {
        split_finish<BM, BN, TM, TN>(p, z, tile, wave, lane, m0, n0, c_zoff, reinterpret_cast<int *>(smem));
    }
}

template <int BM, int BN, int AL, int BL>
int32_t launch(rten_hip_ctx *ctx, const GemmArgs &a, dim3 grid, int mode, double flops, double bytes) {
    char kname[96];
    snprintf(kname, sizeof kname, "igemm_f32_kernel<%d,%d,%d,%d,%d>", BM, BN, AL, BL, mode);
    ProfScope ps(ctx, kname, flops, bytes);
    if (mode == 2) hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, AL, BL, 2>), grid, dim3(NTHREADS), 0, ctx->stream, a);
    else if (mode == 1) hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, AL, BL, 1>), grid, dim3(NTHREADS), 0, ctx->stream, a);
    else hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, AL, BL, 0>), grid, dim3(NTHREADS), 0, ctx->stream, a);
    RTEN_LAUNCH_CHECK(ctx, "igemm_f32_kernel launch");
    return RTEN_HIP_OK;
}

} // namespace

int32_t rten_launch_gemm_f32_reg(rten_hip_ctx *ctx, const void *args, unsigned grid_x, unsigned grid_z, int bm, int bn, int al, int bl, int mode,
                                 double flops, double bytes) {
    TRACED_ARGS(a, args, grid_x * grid_z);
    const dim3 grid(grid_x, grid_z);
    return switch_tile(ctx, "igemm_f32_kernel", bm, bn, [&](auto t) -> int32_t {
        constexpr int BM = decltype(t)::bm, BN = decltype(t)::bn;
        switch (layouts(al, bl)) { // every pair the planner dispatches but the tap-masked gather
        case layouts(A_M4, B_N4): return launch<BM, BN, A_M4, B_N4>(ctx, a, grid, mode, flops, bytes);
        case layouts(A_M4, B_IM2COL): return launch<BM, BN, A_M4, B_IM2COL>(ctx, a, grid, mode, flops, bytes);
        case layouts(A_K4, B_N4): return launch<BM, BN, A_K4, B_N4>(ctx, a, grid, mode, flops, bytes);
        case layouts(A_K4, B_K4): return launch<BM, BN, A_K4, B_K4>(ctx, a, grid, mode, flops, bytes);
        case layouts(A_SCALAR, B_IM2COL): return launch<BM, BN, A_SCALAR, B_IM2COL>(ctx, a, grid, mode, flops, bytes);
        case layouts(A_SCALAR, B_SCALAR): return launch<BM, BN, A_SCALAR, B_SCALAR>(ctx, a, grid, mode, flops, bytes);
        default: return not_covered(ctx, "igemm_f32_kernel");
        }
    });
}
