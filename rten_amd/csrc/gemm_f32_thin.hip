// The thin-tile tail family of the f32 implicit-GEMM kernels (gfx950): split mode 4.  Launch plans: gemm_f32.hip.
#include "gemm_f32_common.h"

namespace {

// =====================================================================================================
// Thin-tile tail kernel: 16 (m) x 64 (n) tiles on v_mfma_f32_16x16x4_f32.
//
// The f32 matrix pipe makes a 32x32 accumulator block x full K a long indivisible unit on one SIMD, and ResNet's column
// counts (batch x 49 x 2^k) leave a fraction of a round of 64x64 tiles over: the chip then idles 12-25 % of the layer's
// time behind a few straggler tiles.  A launch plan with `split_mode == 4` gives the whole rounds to the 64x64 kernel
// (columns [0, n_lo)) and the remaining columns to this kernel, whose waves own 16x16 blocks -- a quarter of the work per
// SIMD, so the tail costs a quarter of a round and every CU takes part.
// v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain like the 32x32x2 form (tools/probes/mfma_16x16x4_order.hip), so an
// output element sees the same chain: depth blocks of 256 folded with separate adds, bias after the first block --
// bit-identical to the big tiles and to the reference.
// Tile DMA as in igemm_f32_dma_kernel (A k-major [K][M4] -> LDS [32][32] with rows >= 16 zero filled, B dense or im2col
// gather -> LDS [32][64]), three stages, k-tiles of 32.  alpha == 1, beta == 0 (convolution) only.
// =====================================================================================================
typedef float f32x4acc __attribute__((ext_vector_type(4)));
constexpr int TBK = 32;               // k-tile depth of the thin kernel
constexpr int TKC_TILES = 256 / TBK;  // k-tiles per reference depth block

template <int BL, bool MULTI_KC>
__global__ __launch_bounds__(NTHREADS, 2) void igemm_f32_thin_kernel(const GemmArgs p) {
    kernarg_prefetch<(int)sizeof(GemmArgs)>();
    static_assert(BL == B_N4 || BL == B_IM2COL || BL == B_IM2COL_TAPS, "thin kernel covers the conv operand layouts");
    constexpr int BM = 16, BN = 64, LDA = 32;        // LDS A image is 32 wide (one dwordx4 DMA instruction per wave), 16 used
    constexpr int STAGE = TBK * (LDA + BN);          // floats per stage
    constexpr int NBV = TBK * BN / 256 / 4;          // dwordx4 per wave per tile (dense B) = 2
    constexpr int NBG = TBK * BN / 64 / 4;           // dword gathers per wave per tile (im2col B) = 8
    constexpr int PER_TILE = 1 + (BL == B_N4 ? NBV : NBG);
    constexpr int NSTAGE = 3;
    constexpr bool IM2COL = BL == B_IM2COL || BL == B_IM2COL_TAPS, TAPS = BL == B_IM2COL_TAPS;
    __shared__ __attribute__((aligned(16))) float smem[NSTAGE * STAGE];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, quad = lane >> 4;
    const int z = blockIdx.y;
    const int tile = blockIdx.x;
    const int bm = tile % p.tiles_m, bn = tile / p.tiles_m; // m fastest: the workgroups of one column strip share the B panel in L2
    const int m0 = bm * BM, n0 = p.n_lo + bn * BN;

    const BatchSlice zs = batch_slice(p, z);
    const long long c_zoff = zs.c_zoff;
    const __amdgpu_buffer_rsrc_t rsA = slice_rsrc(zs.A, p.a_bytes), rsB = slice_rsrc(zs.B, p.b_bytes);
    const int nk = (p.K + TBK - 1) / TBK;

    // A: wave w moves rows [8w, 8w+8) of the k-tile: lane -> (row 8w + lane/8, columns (lane%8)*4 ..+3 of the 32-wide LDS image)
    unsigned a_voff;
    {
        const int k = wave * 8 + (lane >> 3), ml = (lane & 7) * 4, m = m0 + ml;
        a_voff = (ml < BM && m < (int)p.a_cs) ? (unsigned)(((long long)k * p.a_cs + m) * 4) : OOB;
    }
    const unsigned a_kstep = (unsigned)(TBK * p.a_cs * 4);

    [[maybe_unused]] unsigned b_voff[BL == B_N4 ? NBV : 1];
    [[maybe_unused]] int b_krow[BL == B_N4 ? NBV : 1];
    [[maybe_unused]] unsigned b_kstep = 0;
    [[maybe_unused]] int im_iy0 = 0, im_ix0 = 0, im_pix = 0;
    [[maybe_unused]] unsigned im_inv = 0;
    if constexpr (BL == B_N4) {
        dma_b_offsets<BN, NBV>(p, n0, wave, lane, b_voff, b_krow);
        b_kstep = (unsigned)(TBK * p.b_rs * 4);
    } else {
        im2col_column<TAPS>(p, n0 + lane, im_iy0, im_ix0, im_pix, im_inv); // gather instruction = one k row x 64 columns: a lane sees one column
    }

    typedef const __attribute__((address_space(4))) i32x2 *lut_ptr_t;
    constexpr int LROWS = TBK / 4; // rows of a k-tile gathered by one wave
    [[maybe_unused]] i32x2 lutE[LROWS];
    [[maybe_unused]] auto fetch_lut = [&](int kt) {
        if constexpr (IM2COL) {
            const int krow0 = kt * TBK + wave * LROWS;
            const lut_ptr_t lc = (lut_ptr_t)(unsigned long long)p.lut;
#pragma unroll
            for (int j = 0; j < LROWS; j++) lutE[j] = lc[krow0 + j];
        }
    };

    typedef __attribute__((address_space(3))) void *lds_ptr_t;
    auto issue_tile = [&](int kt, int stage) {
        float *As = smem + stage * STAGE;
        float *Bs = As + TBK * LDA;
        const int kts = kt < nk ? kt : (nk > 0 ? nk - 1 : 0); // keep the scalar offset inside the buffer
        const bool past = kt >= nk;
        // rows >= K lie past the end of the [K][M4] buffer: the hardware range check zero-fills them
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_t)(As + wave * 256), 16, (int)(past ? OOB : a_voff), (int)((unsigned)kts * a_kstep), 0, 0);
        if constexpr (BL == B_N4) {
            const int kleft = p.K - kt * TBK;
            const unsigned b_soff = (unsigned)kts * b_kstep;
#pragma unroll
            for (int j = 0; j < NBV; j++)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr_t)(Bs + (wave * NBV + j) * 256), 16, (int)(b_krow[j] < kleft ? b_voff[j] : OOB), (int)b_soff, 0, 0);
        } else {
#pragma unroll
            for (int r = 0; r < NBG; r++) {
                const i32x2 e = lutE[r];
                unsigned voff;
                if constexpr (TAPS) {
                    voff = ((im_inv << e[1]) & 0x80000000u) | ((unsigned)(im_pix + e[0]) << 2);
                } else {
                    const int iy = im_iy0 + (e[1] & 0xffff);
                    const int ix = im_ix0 + (e[1] >> 16);
                    const bool ok = ((unsigned)iy < (unsigned)p.H) & ((unsigned)ix < (unsigned)p.W);
                    voff = ok ? (unsigned)(im_pix + e[0]) << 2 : OOB;
                }
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr_t)(Bs + (wave * LROWS + r) * BN), 4, (int)voff, 0, 0, 0);
            }
        }
    };

    const int wq = t >> 6;       // per-lane copy of the wave id for address math
    const int wn0 = wq * 16;     // the four waves own 16-column strips of the 64-column tile
    f32x4acc acc = {0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] f32x4acc tot = {0.f, 0.f, 0.f, 0.f};

    auto compute_tile = [&](int stage) {
        // fragments of k-step kk (4 rows of the tile): A[m = l15][k = 4 kk + quad], B[k = 4 kk + quad][n = wn0 + l15]
        const float *As = smem + stage * STAGE + quad * LDA + l15;
        const float *Bs = smem + stage * STAGE + TBK * LDA + quad * BN + wn0 + l15;
        float af[TBK / 4], bf[TBK / 4];
#pragma unroll
        for (int kk = 0; kk < TBK / 4; kk++) {
            af[kk] = As[kk * 4 * LDA];
            bf[kk] = Bs[kk * 4 * BN];
        }
#pragma unroll
        for (int kk = 0; kk < TBK / 4; kk++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[kk], bf[kk], acc, 0, 0, 0);
    };

    // element r of the accumulator: row m0 + 4 * quad + r, column n0 + wn0 + l15
    const __amdgpu_buffer_rsrc_t rsBias = __builtin_amdgcn_make_buffer_rsrc((void *)((p.bias ? p.bias : p.C) + (long long)z * p.bias_bs), 0, 0x7ffffffc, 0x00020000);
    auto first_block = [&](f32x4acc a) { // alpha == 1, beta == 0: out = acc, then the bias (rten-gemm/src/lib.rs:1008-1013,1221-1255)
        f32x4acc v = a;
        if (p.bias_kind == RTEN_HIP_BIAS_PER_ROW) {
            float b4[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = m0 + 4 * quad + r;
                b4[r] = buf_load1(rsBias, m < p.M ? (unsigned)m << 2 : OOB, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) v[r] = v[r] + b4[r];
        }
        return v;
    };

    const int nblk = MULTI_KC ? (nk + TKC_TILES - 1) / TKC_TILES : 1;
    fetch_lut(0);
#pragma unroll
    for (int i = 0; i < NSTAGE - 1; i++) {
        issue_tile(i, i);
        fetch_lut(i + 1);
    }
    int stage = 0;
    for (int blk = 0; blk < nblk; blk++) {
        const int kt_end = MULTI_KC ? ((blk + 1) * TKC_TILES < nk ? (blk + 1) * TKC_TILES : nk) : nk;
        for (int kt = blk * TKC_TILES; kt < kt_end; kt++) {
            wait_vmcnt<PER_TILE *(NSTAGE - 2)>();
            __builtin_amdgcn_s_barrier();
            const int stp = stage == 0 ? NSTAGE - 1 : stage - 1;
            issue_tile(kt + NSTAGE - 1, stp);
            fetch_lut(kt + NSTAGE);
            compute_tile(stage);
            stage = stage == NSTAGE - 1 ? 0 : stage + 1;
        }
        if constexpr (MULTI_KC) {
            if (blk + 1 < nblk) {
                if (blk == 0) tot = first_block(acc);
                else {
#pragma unroll
                    for (int r = 0; r < 4; r++) tot[r] = tot[r] + acc[r];
                }
                acc = f32x4acc{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    wait_vmcnt<0>(); // drain the look-ahead tiles before the LDS goes away

    f32x4acc v;
    if constexpr (MULTI_KC) { // launched only for K > 256: at least two depth blocks
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = tot[r] + acc[r];
    } else {
        v = first_block(acc);
    }
    // residual Add, activation, NCHW / row-major store
    const int n = n0 + wn0 + l15;
    const bool cok = n < p.N;
    const int nn = cok ? n : 0;
    const int nb = nn / p.Pn, np = nn - nb * p.Pn;
    const unsigned col = (unsigned)((long long)nb * p.c_ns + np);
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void *)(p.C + c_zoff), 0, 0x7ffffffc, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc((void *)((p.res ? p.res : p.C) + c_zoff), 0, 0x7ffffffc, 0x00020000);
    unsigned voff[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int m = m0 + 4 * quad + r;
        voff[r] = (cok && m < p.M) ? (col + (unsigned)m * (unsigned)p.c_rs) << 2 : OOB;
    }
    if (p.res != nullptr) {
        float rr[4];
#pragma unroll
        for (int r = 0; r < 4; r++) rr[r] = buf_load1(rsR, voff[r], 0);
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = v[r] + rr[r];
    }
    if (p.act == RTEN_HIP_ACT_RELU) {
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = vm::relu(v[r]);
    } else if (p.act == RTEN_HIP_ACT_GELU) {
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = vm::gelu(v[r]);
    } else if (p.act != RTEN_HIP_ACT_NONE) {
        vm::activation_n<4>(p.act, v, p.act_a, p.act_b);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float x = v[r];
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x), rsC, (int)voff[r], 0, 0);
    }
}

template <int BL>
int32_t launch_thin(rten_hip_ctx *ctx, const GemmArgs &a, unsigned grid_x, bool multi, double flops, double bytes) {
    char kname[96];
    snprintf(kname, sizeof kname, "igemm_f32_thin_kernel<%d,%s>", BL, multi ? "true" : "false");
    ProfScope ps(ctx, kname, flops, bytes);
    if (multi) hipLaunchKernelGGL((igemm_f32_thin_kernel<BL, true>), dim3(grid_x, 1u), dim3(NTHREADS), 0, ctx->stream, a);
    else hipLaunchKernelGGL((igemm_f32_thin_kernel<BL, false>), dim3(grid_x, 1u), dim3(NTHREADS), 0, ctx->stream, a);
    RTEN_LAUNCH_CHECK(ctx, "igemm_f32_thin_kernel launch");
    return RTEN_HIP_OK;
}

} // namespace

int32_t rten_launch_gemm_f32_thin(rten_hip_ctx *ctx, const void *args, unsigned grid_x, int bl, int multi, double flops, double bytes) {
    const GemmArgs &a = *static_cast<const GemmArgs *>(args);
    switch (bl) {
    case B_N4: return launch_thin<B_N4>(ctx, a, grid_x, multi != 0, flops, bytes);
    case B_IM2COL: return launch_thin<B_IM2COL>(ctx, a, grid_x, multi != 0, flops, bytes);
    case B_IM2COL_TAPS: return launch_thin<B_IM2COL_TAPS>(ctx, a, grid_x, multi != 0, flops, bytes);
    default: return not_covered(ctx, "igemm_f32_thin_kernel");
    }
}
