// The small-M weight-streaming family of the f32 GEMM kernels (gfx950): GEMM variant 31, and the automatic choice for one batch with M <= 64.
// Its fold / epilogue (fold_first16, fold_next16, store_out16) lives in gemm_f32_common.h.
#include "gemm_f32_common.h"

namespace {

// =====================================================================================================
// Small-M weight streaming (variant 31; the automatic choice for M <= 64, one batch): the classifier / projection shape, where the
// tiled kernels have a handful of 64-row tiles and one of them streams megabytes of B alone (ResNet-50's 32 x 2048 x 1000 Gemm:
// 16 workgroups, 19-25 us for an 8 MB weight read).  Here a WAVE owns one 16x16 block of C for ONE depth block (kc = 256): a chain of
// 64 dependent v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain, tools/probes/mfma_16x16x4_order.hip) -- the reference's micro-kernel
// chain for that block (rten-gemm/src/kernels/simd_generic.rs:326-367) -- and a workgroup = 4 such waves sharing 16 * MT rows of A and
// 64 / MT * 16 columns of B through LDS.  grid = column groups x depth blocks, so ceil(N / (64 / MT * 16)) * ceil(K / 256) workgroups stream B
// (classifier: 32 x 8 = 256, one per compute unit, 64 KB each).  The raw block sums go to the split-K slab; the last workgroup of
// a 16x16 block to arrive folds them in depth-block order (first block: beta * C + bias; later blocks: separate adds;
// rten-gemm/src/lib.rs:1008-1013,1221-1255) -- same bits as the unsplit chain, same visibility protocol as split_finish.
//
// LDS image of an operand row (an A row or a B column; 256 depths = 1 KB): depth k = 16 j + 4 i + g stored at 16 j + 4 g + i, the 16-byte groups of a
// row XOR-swizzled by the row (sm_at): lane (row = lane % 16, g = lane / 16) reads the operands of its MFMAs 4 j .. 4 j + 3 with ONE conflict-free
// ds_read_b128, a loader lane holding depths 16 j + 4 q + {0..3} of a row writes four words (conflict free), and 64 or 80 rows are 64 / 80 KB:
// TWO workgroups per compute unit, so one's operand fetch runs under the other's MFMA chain.
// =====================================================================================================
constexpr int SM_LD = 256;
// float index of (operand row, position in the row's image): 16-byte groups XOR-swizzled by the row so that 16 rows at one position fall on 16 different bank groups
__device__ __forceinline__ int sm_at(int row, int pos) { return row * SM_LD + (pos ^ ((row & 15) << 2)); }

template <int MT>
__global__ __launch_bounds__(256) void gemm_f32_smallm_kernel(const GemmArgs p) {
    kernarg_prefetch<(int)sizeof(GemmArgs)>();
    constexpr int NW = 4 / MT;               // 16-column blocks per workgroup
    constexpr int RA = 16 * MT, RB = 16 * NW; // operand rows in LDS
    __shared__ __attribute__((aligned(16))) float smem[(RA + RB) * SM_LD];
    float *As = smem, *Bs = smem + RA * SM_LD;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, quad = lane >> 4;
    const int gx = blockIdx.x, kb = blockIdx.y;
    const int n0 = gx * RB, k0 = kb * 256;
    const int depth = p.K - k0 < 256 ? p.K - k0 : 256;
    const int nblk = (int)gridDim.y;

    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void *)p.A, 0, (int)p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void *)p.B, 0, (int)p.b_bytes, 0x00020000);

    // ---- stage the operands: depth-contiguous rows take 16-byte loads (a wave covers 16 rows x 64 bytes per depth group j)
    const bool a_vec = p.tiles_m & 1, b_vec = p.tiles_m & 2; // set by the launcher: depth stride 1, row stride and K multiples of 4, base 16-byte aligned
    if (a_vec) {
        f32x4 v[MT * 4];
#pragma unroll
        for (int u = 0; u < MT * 4; u++) {
            const int f = u * 256 + t, q = f & 3, r = (f >> 2) & 15, j = (f >> 6) & 15, rg = f >> 10;
            const int row = rg * 16 + r, k = 16 * j + 4 * q;
            v[u] = buf_load4(rsA, (row < p.M && k < depth) ? (unsigned)(((long long)row * p.a_rs + k0 + k) << 2) : OOB, 0);
        }
#pragma unroll
        for (int u = 0; u < MT * 4; u++) {
            const int f = u * 256 + t, q = f & 3, r = (f >> 2) & 15, j = (f >> 6) & 15, rg = f >> 10;
            const int row = rg * 16 + r;
            As[sm_at(row, 16 * j + q)] = v[u][0]; As[sm_at(row, 16 * j + 4 + q)] = v[u][1]; As[sm_at(row, 16 * j + 8 + q)] = v[u][2]; As[sm_at(row, 16 * j + 12 + q)] = v[u][3];
        }
    } else if (p.tiles_m & 4) { // A given transposed ([K][M], 16-byte groups of rows): a wave covers 16 depths x 16 rows per load
        f32x4 v[MT * 4];
#pragma unroll
        for (int u = 0; u < MT * 4; u++) {
            const int f = u * 256 + t, c4 = f & 3, k = 16 * ((f >> 6) & 15) + ((f >> 2) & 15), row = 16 * (f >> 10) + 4 * c4;
            v[u] = buf_load4(rsA, (row < p.M && k < depth) ? (unsigned)(((long long)(k0 + k) * p.a_cs + row) << 2) : OOB, 0);
        }
#pragma unroll
        for (int u = 0; u < MT * 4; u++) {
            const int f = u * 256 + t, c4 = f & 3, k = 16 * ((f >> 6) & 15) + ((f >> 2) & 15), row = 16 * (f >> 10) + 4 * c4;
            const int pos = (k & ~15) + 4 * (k & 3) + ((k >> 2) & 3);
            As[sm_at(row, pos)] = v[u][0]; As[sm_at(row + 1, pos)] = v[u][1]; As[sm_at(row + 2, pos)] = v[u][2]; As[sm_at(row + 3, pos)] = v[u][3];
        }
    } else {
        const bool along_m = p.a_dir_m; // rows are the contiguous direction (A given transposed): lanes walk rows
#pragma unroll 8
        for (int u = 0; u < RA; u++) {
            const int idx = u * 256 + t;
            const int row = along_m ? idx % RA : idx >> 8, k = along_m ? idx / RA : idx & 255;
            const float x = buf_load1(rsA, (row < p.M && k < depth) ? (unsigned)(((long long)row * p.a_rs + (long long)(k0 + k) * p.a_cs) << 2) : OOB, 0);
            As[sm_at(row, (k & ~15) + 4 * (k & 3) + ((k >> 2) & 3))] = x;
        }
    }
    if (b_vec) {
        f32x4 v[NW * 4];
#pragma unroll
        for (int u = 0; u < NW * 4; u++) {
            const int f = u * 256 + t, q = f & 3, r = (f >> 2) & 15, j = (f >> 6) & 15, rg = f >> 10;
            const int col = n0 + rg * 16 + r, k = 16 * j + 4 * q;
            v[u] = buf_load4(rsB, (col < p.N && k < depth) ? (unsigned)(((long long)col * p.b_cs + k0 + k) << 2) : OOB, 0);
        }
#pragma unroll
        for (int u = 0; u < NW * 4; u++) {
            const int f = u * 256 + t, q = f & 3, r = (f >> 2) & 15, j = (f >> 6) & 15, rg = f >> 10;
            const int row = rg * 16 + r;
            Bs[sm_at(row, 16 * j + q)] = v[u][0]; Bs[sm_at(row, 16 * j + 4 + q)] = v[u][1]; Bs[sm_at(row, 16 * j + 8 + q)] = v[u][2]; Bs[sm_at(row, 16 * j + 12 + q)] = v[u][3];
        }
    } else if (p.tiles_m & 8) { // B as [K][N] (16-byte groups of columns): a wave covers 16 depths x 16 columns per load
        f32x4 v[NW * 4];
#pragma unroll
        for (int u = 0; u < NW * 4; u++) {
            const int f = u * 256 + t, c4 = f & 3, k = 16 * ((f >> 6) & 15) + ((f >> 2) & 15), c = 16 * (f >> 10) + 4 * c4;
            v[u] = buf_load4(rsB, (n0 + c < p.N && k < depth) ? (unsigned)(((long long)(k0 + k) * p.b_rs + n0 + c) << 2) : OOB, 0);
        }
#pragma unroll
        for (int u = 0; u < NW * 4; u++) {
            const int f = u * 256 + t, c4 = f & 3, k = 16 * ((f >> 6) & 15) + ((f >> 2) & 15), c = 16 * (f >> 10) + 4 * c4;
            const int pos = (k & ~15) + 4 * (k & 3) + ((k >> 2) & 3);
            Bs[sm_at(c, pos)] = v[u][0]; Bs[sm_at(c + 1, pos)] = v[u][1]; Bs[sm_at(c + 2, pos)] = v[u][2]; Bs[sm_at(c + 3, pos)] = v[u][3];
        }
    } else {
        const bool along_n = p.b_dir_n; // columns are the contiguous direction (B as [K][N]): lanes walk columns
#pragma unroll 8
        for (int u = 0; u < RB; u++) {
            const int idx = u * 256 + t;
            const int c = along_n ? idx % RB : idx >> 8, k = along_n ? idx / RB : idx & 255;
            const int col = n0 + c;
            const float x = buf_load1(rsB, (col < p.N && k < depth) ? (unsigned)(((long long)(k0 + k) * p.b_rs + (long long)col * p.b_cs) << 2) : OOB, 0);
            Bs[sm_at(c, (k & ~15) + 4 * (k & 3) + ((k >> 2) & 3))] = x;
        }
    }
    __syncthreads();

    // ---- one 16x16 block of C, one depth block: the MFMA chain
    const int mt = wave % MT, nw = wave / MT;
    f32x4 af[16], bf[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        af[j] = *(const f32x4 *)(As + sm_at(mt * 16 + l15, 16 * j + 4 * quad));
        bf[j] = *(const f32x4 *)(Bs + sm_at(nw * 16 + l15, 16 * j + 4 * quad));
    }
    f32x4v acc[1][1];
    acc[0][0] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 16; j++) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (16 * j + 4 * i < depth) // (uniform; depths past the end inside the last MFMA are zeros: exact)
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j][i], bf[j][i], acc[0][0], 0, 0, 0);
        }
    }

    const int mb = mt * 16 + 4 * quad, nb0 = n0 + nw * 16 + l15;
    if (nblk == 1) {
        fold_first16<1, 1>(p, 0, acc, acc, mb, nb0, 0);
        store_out16<1, 1>(p, acc, mb, nb0, 0);
        return;
    }
    // ---- park the raw sums; the last arrival of the column group folds them in depth-block order
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(p.slab + (long long)gx * nblk * 1024), 0, nblk * 4096, 0x00020000);
    coherent_store4(rs, (unsigned)((kb * 4 + wave) * 64 + lane) * 16u, acc[0][0]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's write-through store has been acknowledged
    // per-WAVE arrival (counter gx * 4 + wave): the nblk waves that own the same 16x16 block meet on it, no workgroup barrier on the way
    unsigned old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(p.split_counters + gx * 4 + wave, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != (unsigned)nblk - 1u) return;
    // all of a batch's slots are in flight before the first fold (one memory round trip per 8 depth blocks, not one per block)
    f32x4v tot[1][1], cur[1][1];
    f32x4 part[8];
    for (int s0 = 0; s0 < nblk; s0 += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) part[u] = coherent_load4(rs, s0 + u < nblk ? (unsigned)(((s0 + u) * 4 + wave) * 64 + lane) * 16u : OOB);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (s0 + u < nblk) {
                cur[0][0] = part[u];
                if (s0 + u == 0) fold_first16<1, 1>(p, 0, cur, tot, mb, nb0, 0);
                else fold_next16<1, 1>(p, cur, tot);
            }
        }
    }
    store_out16<1, 1>(p, tot, mb, nb0, 0);
    if (lane == 0) p.split_counters[gx * 4 + wave] = 0u;
}

} // namespace

int32_t rten_launch_gemm_f32_smallm(rten_hip_ctx *ctx, const void *args, const rten_hip_gemm_desc *d, const float *ap, const float *bp) {
    GemmArgs a = *static_cast<const GemmArgs *>(args);
    if (d->batch != 1 || d->m > 64 || d->k <= 0) return RTEN_HIP_ERR_UNSUPPORTED;
    const int MT = d->m <= 16 ? 1 : d->m <= 32 ? 2 : 4, RB = 16 * (4 / MT);
    const long long gx = (d->n + RB - 1) / RB, nblk = (d->k + 255) / 256;
    if (gx > 0x7fffffff || nblk > 65535) return RTEN_HIP_ERR_UNSUPPORTED;
    if (nblk > 1) {
        if (!ctx->split_counters || gx * 4 > rten_hip_ctx::kSplitCounters) return RTEN_HIP_ERR_UNSUPPORTED;
        char *sc = (char *)rten_scratch(ctx, 4096 + (size_t)gx * (size_t)nblk * 4096);
        // (growing the slab is impossible while a capture is active: decline, the tiled kernels run the product -- ADVICE round 5)
        if (!sc) return ctx->capturing ? RTEN_HIP_ERR_UNSUPPORTED : rten_set_error(ctx, RTEN_HIP_ERR_HIP, "split-K slab allocation failed");
        a.slab = (float *)(sc + 4096);
        a.split_counters = ctx->split_counters;
    }
    const bool k4 = d->k % 4 == 0;
    // loader forms (16-byte loads): bit 0 / 1 = A / B depth-contiguous; bit 2 / 3 = A rows / B columns contiguous
    a.tiles_m = ((d->a_cs == 1 && d->a_rs % 4 == 0 && k4 && aligned16(ap)) ? 1 : 0) | ((d->b_rs == 1 && d->b_cs % 4 == 0 && k4 && aligned16(bp)) ? 2 : 0);
    if (!(a.tiles_m & 1) && d->a_rs == 1 && d->a_cs % 4 == 0 && d->m % 4 == 0 && aligned16(ap)) a.tiles_m |= 4;
    if (!(a.tiles_m & 2) && d->b_cs == 1 && d->b_rs % 4 == 0 && d->n % 4 == 0 && aligned16(bp)) a.tiles_m |= 8;
    char kname[64];
    snprintf(kname, sizeof kname, "gemm_f32_smallm_kernel<%d>", MT);
    ProfScope ps(ctx, kname, 2.0 * d->m * (double)d->n * d->k, 4.0 * ((double)d->m * d->k + (double)d->k * d->n + (double)d->m * d->n));
    const dim3 grid((unsigned)gx, (unsigned)nblk);
    if (MT == 1) hipLaunchKernelGGL((gemm_f32_smallm_kernel<1>), grid, dim3(256), 0, ctx->stream, a);
    else if (MT == 2) hipLaunchKernelGGL((gemm_f32_smallm_kernel<2>), grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL((gemm_f32_smallm_kernel<4>), grid, dim3(256), 0, ctx->stream, a);
    RTEN_LAUNCH_CHECK(ctx, "gemm_f32_smallm_kernel launch");
    return RTEN_HIP_OK;
}
