// Fast int8 GEMM / convolution path for gfx950: v_mfma_i32_32x32x32_i8 fed by 16-byte LDS-DMA.
//
// Replaces (together with int8.hip, which stays as the generic fallback): GemmExecutor<u8,i8,i32> and its packing
// (rten-gemm/src/kernels/generic.rs:274-366, packing/int8.rs), the int8 im2col (im2col.rs:264-389) and the
// front-ends conv_integer / ConvIntegerToFloat / matmul_integer (src/ops/conv.rs:421-587, matmul.rs:582-810).
//
// Integer sums are exact in any order, so -- unlike the f32 path -- the K dimension may be re-ordered.  That is
// what makes the int8 path fast on this machine:
//   * Both MFMA operands want 16 CONSECUTIVE k bytes per lane.  Operands are therefore staged once per call as
//     CHUNK-MAJOR signed bytes [K/16][rows][16 B]: weights with k = (ky, kx, c) (channels padded to 16) plus their row
//     sums; conv activations as a zero-point-PADDED channel-blocked image [N][Cp/16][H+pads][W+pads][16 B], so that
//     the im2col gather of one (tap, 16-channel) chunk is one aligned 16-byte load per pixel and needs no bounds tests
//     at all (the spatial border holds the reference's padding value for the selected pad mode).
//     Chunk-major (rather than k-contiguous rows) because the 64 lanes of one tile-DMA instruction then read ONE
//     1 KiB run (GEMM) or a few row-long runs (conv) instead of 64 pieces a row pitch apart: with a power-of-two
//     pitch those 64 pieces fall on 2-4 of the 16 L2 channels (measured: +8 % end to end on ResNet-50 int8).
//     u8 operands move to the signed domain (x ^ 0x80) during staging; (x - zp) is invariant under that shift.
//   * Main loop: tiles go L2 -> LDS with `buffer_load_dwordx4 ... lds` (1 KiB per wave instruction), chunk-major
//     LDS image [4 chunks][rows][16 B] (the DMA's lane-linear destination), so an MFMA operand fetch is one
//     conflict-free ds_read_b128.  Three LDS stages, counted vmcnt waits, one barrier per 64-byte k-tile.
//     Per-lane offsets are loop invariant; the k advance (conv: the (ky, kx, c) chunk walk) is scalar.
//     What bounds it (tools/probes/lds_fill_rate.hip, ablation in DESIGN.md section 7): the tile DMA of a workgroup,
//     not the MFMAs -- hence the tile / tile-order rules in dispatch_fast.
//   * Zero-point algebra of the reference (simd_generic.rs:676-746): C = dot - b_zp*rowsum(A) - a_zp*colsum(B)
//     + K*a_zp*b_zp with weight sums from the staging pass; the activation-side sums are only accumulated
//     (v_dot4 on the operand fragments) when the weight zero point can be non-zero.
//   * Epilogue fuses cast_scale, bias, residual Add and Relu; i32 or f32 output straight into NCHW / row-major.
//   * A launch of this path is usually ONE wave of workgroups (a few hundred tiles for 256 CUs), so its prologue and epilogue are on the critical path one
//     for one (tools/debug/i8_trace.py on a -DRTEN_TRACE build).  Hence: all kernel-argument lines requested at entry
//     (kernarg_prefetch), index arithmetic by multiply-shift (rten_div), no arithmetic on a loaded value before the main loop (it would drain the
//     vector-memory counter in front of the first operand request), the launch's single activation zero point through the scalar cache, and the
//     single-row-term epilogue of the convolution form as a template flag (RT).
// This unit: the kernel and the dispatch of its launch forms (int8_fast.h: the other two units of the path and what they share).
#include <array>
#include <cstdlib>
#include <cstring>

#include "int8_fast.h"
#include "quantize.h"
#include "vecmath.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

namespace {

constexpr unsigned OOB = 0x80000000u;

// A zero point in the signed domain, in two steps: the load (raw byte, -1 = no zero-point input) is issued in the kernel's prologue, the conversion waits until the epilogue --
// any arithmetic on the loaded byte makes the compiler drain every outstanding load right there, a full memory round trip before the first operand tile
// is even requested (tools/debug/i8_trace.py: ~1000 cycles per launch).
__device__ __forceinline__ int zp_raw(const uint8_t *zp, int idx) { return zp ? (int)zp[idx] : -1; }
__device__ __forceinline__ int zp_from_raw(int raw, int is_signed) {
    if (raw < 0) return is_signed ? 0 : -128;
    return is_signed ? (int)(int8_t)(uint8_t)raw : raw - 128;
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ constexpr int acc_row(int r) { return (r & 3) + 8 * (r >> 2); }

// ---------------------------------------------------------------------------------------------------------
// main kernel
// ---------------------------------------------------------------------------------------------------------
// RES: the epilogue adds a residual tile (prefetched into 16 * TM * TN registers); a separate instantiation so that the
// launches without one keep the smaller register footprint (one more workgroup per CU on the 128 x 128 tile).
// KTK = k bytes per tile (a multiple of 64): one barrier, one counted wait and one trip round the loop per KTK / 32 MFMA steps.
// The i8 matrix pipe retires a 32x32x32 step in 32 cycles -- sixteen times the f32 rate -- so with 64-byte k-tiles a wave's two
// MFMAs (64 cycles) sat behind ~600 cycles of barrier / wait / DMA issue / loop overhead (tools/probes/kloop.hip prices that
// overhead for the f32 loop); the long-K launches of stages 2-3 therefore take 256-byte k-tiles.  All LDS is ONE dynamic array.
extern __shared__ __attribute__((aligned(16))) uint8_t i8_smem[];

// KG = k-groups: the workgroup has KG x 4 waves; group g takes k-tiles g, g + KG, ... into accumulators of its own, and the
// groups' partial sums are added through LDS before the (group 0) epilogue -- exact, integer addition is order-free.  An
// under-filled launch (stage 3-4 of ResNet-50 at batch 32: ~200 tiles of 64 x 64 for 256 CUs) otherwise runs ONE wave per
// SIMD, and every latency of its k-loop (barrier, DMA issue, LDS fragment reads, dependent MFMAs: ~550 cycles per 64-byte
// k-tile, independent of where the operands come from -- profiles/r05/int8_kloop_ablation.txt) is exposed 72 times in a row.
// BQ = the B operand is QUANTIZED ON LOAD from the f32 activation tensor (pointwise stride-1 unpadded convolutions of a dynamically
// quantized graph): DynamicQuantizeLinear's parameters come from the min/max block the producing conv accumulated, a thread
// reads 16 channels of one pixel (lanes = consecutive pixels: 256-byte runs), converts with dql::quant_u8 and writes the
// 16-byte chunk piece the DMA would have delivered (conflict-free ds_write_b128).  The staging launch, its 1 B/element write
// and the staged image's read disappear; A still arrives by LDS-DMA.  Same codes, same sums: bit-identical.
// QO = the output is QUANTIZED IN THE EPILOGUE for the one convolution that consumes it (DynamicQuantizeLinear -> ConvInteger of the
// next layer, src/ops/quantize.rs:352-436): the finished f32 values stay in the accumulator registers, every workgroup publishes its
// min / max (the ordered-uint slots of the producer-statistics scheme) and arrives on a grid-wide counter barrier; behind it each
// workgroup folds the slots -- min / max are order free, so these are the statistics of the two-sweep operator -- derives the same
// scale / zero point, converts with the same dql::quant_u8 and writes the codes straight into the consumer's staged image
// (channel-blocked, padded; border pieces included).  The f32 tensor is written only if somebody else needs it (p.C != NULL).
// Every workgroup of the grid must be resident at once (the host checks the occupancy before it launches this form).
// (the exchange block's layout, kSyncCtlWords / kSyncGranules / kSyncWords: int8_fast.h)
constexpr unsigned long long kGranuleReset = 0x00000000ffffffffull; // {min = 0xffffffff, max = 0}: what a reset leaves, never a real pair
constexpr unsigned kSyncSpinLimit = 1u << 17;
// KS = cross-workgroup K split (round 6): the launches of stages 2-3 at batch 32 are 52-392 tiles for 256 compute units with 16-72 k-tiles each -- a
// k-loop of 6-15 thousand cycles on a chip that is mostly empty.  With KS the grid is tiles x p.ks workgroups; part q of a tile walks k-tiles
// [q * nkt / ks, (q + 1) * nkt / ks), parks its raw int32 accumulators (write-through stores, as the f32 split-K slab) and arrives on the tile's counter;
// the last arrival reads the other parts back (L2-bypassing loads), adds them to its own registers and runs the unchanged epilogue.  Integer sums are
// exact in any order: same bits whichever workgroup arrives last (tests: 200 launches, every split count).
// QO == 2 = the RECOMPUTE form of a quantized output (round 6): the launch before this one ran the same convolution with `no_store` and left the output's
// min / max in the statistics block (p.in_stats); this launch folds the block in its prologue (as a BQ kernel does), computes the tile again and writes
// the codes straight into the consumer's staged image.  No grid-wide exchange, no residency requirement, no time-out: replicas side by side ("lanes") may
// use it, where the i8 pipe is 3-6 % busy and the step is bound by HBM bytes -- the f32 tensor of a single-consumer edge (4 B written + 4 B read back per
// element) never exists.  Same statistics (min / max are order-free), same dql_params, same quant_u8: the codes of the two-launch sequence.
template <int BM, int BN, int NSTAGE, bool RES, int KTK = 64, int KG = 1, bool BQ = false, int QO = 0, bool RT = false, bool KS = false>
__global__ __launch_bounds__(256 * KG, KG == 1 ? 2 : 1) void igemm_i8_fast_kernel(const FastArgs p) {
    static_assert(!KS || (KG == 1 && !BQ && !QO && !RES && RT && KTK == 64), "cross-workgroup K split: the plain single-row-term convolution form only");
    static_assert(!BQ || (KG == 1 && KTK == 64), "quantize-on-load: one k-group, 64-byte k-tiles");
    static_assert(!(BQ && QO), "quantize-on-load and quantized output are separate instantiations");
    constexpr int WM = 2, WN = 2;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int RA = BM / 64, RB = BN / 64;      // DMA instructions per chunk (64 rows each)
    constexpr int CPW = KTK / 64;                  // chunks per wave per tile: wave w moves chunks w, w + 4, ... of the tile
    constexpr int PER_TILE = (RA + RB) * CPW;
    constexpr int SUB = (BM + BN) * KTK;           // bytes of one k-tile
    constexpr int STAGE = SUB * KG;                // a stage holds one k-tile per group
    uint8_t *const smem = i8_smem;
    kernarg_prefetch<(int)sizeof(FastArgs)>(); // (7 lines)

    const int t = threadIdx.x, lane = t & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane(t >> 6); // 0 .. 4 KG - 1
    const int kg = wave_all >> 2;                                // k-group of this wave
    const int wave = wave_all & 3;                               // wave within the group: its chunk slot and its quadrant of the tile
    const int wq = wave;
    const int l31 = lane & 31, half = lane >> 5;
#ifdef RTEN_TRACE // build.sh -DRTEN_TRACE: cycle stamps at the phase boundaries, printed by one wave (tools/debug/i8_trace.py)
    unsigned long long tr_seg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tr_prev = __builtin_readcyclecounter();
    const unsigned long long tr_c0 = tr_prev, tr_r0 = __builtin_amdgcn_s_memrealtime(); // (100 MHz: cycles per tick x 100 = the shader clock in MHz during this workgroup)
#define I8_STAMP(i) { const unsigned long long now_ = __builtin_readcyclecounter(); tr_seg[i] += now_ - tr_prev; tr_prev = now_; }
#else
#define I8_STAMP(i)
#endif
    int tile;
    [[maybe_unused]] int ks_part = 0;
    {
        const int nt = gridDim.x, id = blockIdx.x;
        const int xcd = id & 7, q = nt >> 3, r = nt & 7;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
        if constexpr (KS) { // an XCD's run of consecutive indices walks neighbouring tiles of ONE K slice: they share that slice of the operand panels
            const int ntiles = p.tiles_m * p.tiles_n;
            ks_part = tile / ntiles;
            tile -= ks_part * ntiles;
        }
    }
    const int tdiv = p.n_fastest ? p.tiles_n : p.tiles_m, tq = rten_div(tile, p.d_tile), tr = tile - tq * tdiv;
    const int bm = p.n_fastest ? tq : tr, bn = p.n_fastest ? tr : tq;
    const int m0 = bm * BM, n0 = bn * BN;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void *)p.A, 0, (int)p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(BQ ? (void *)p.xf : (void *)p.B, 0, (int)p.b_bytes, 0x00020000);

    // loop-invariant per-lane row bases (bytes)
    unsigned a_voff[RA], b_voff[RB];
#pragma unroll
    for (int j = 0; j < RA; j++) {
        const int m = m0 + j * 64 + lane;
        a_voff[j] = m < p.M ? (unsigned)m * 16u : OOB;
    }
#pragma unroll
    for (int j = 0; j < RB; j++) {
        const int n = n0 + j * 64 + lane;
        if (n < p.N) {
            if (RT || p.conv) { // (RT kernels are convolutions by construction: the GEMM form is not compiled into them)
                const int nb = rten_div(n, p.d_pn), np = n - nb * p.Pn;
                const int oy = rten_div(np, p.d_ow), ox = np - oy * p.OW;
                b_voff[j] = (unsigned)(((nb * (p.Cp / 16) * p.Hp + oy * p.sy) * p.Wp + ox * p.sx) * 16);
            } else {
                b_voff[j] = (unsigned)n * 16u;
            }
        } else {
            b_voff[j] = OOB;
        }
    }

    I8_STAMP(0) // kernel arguments, tile decode, per-lane row / pixel bases
    // ---- this wave's chunk walk: chunk index wave, wave + 4, ... of the K axis (16-byte chunks).
    // The B-side scalar offset of a chunk -- conv: its (ky, kx, c16) position on the padded image -- comes from a table that the
    // workgroup builds in LDS before the loop (one division pair per chunk, once), and everything the loop derives from the
    // walk is kept in scalar registers: the previous form carried an odometer in vector registers and paid ~100 VALU + SALU
    // instructions per k-tile, waterfall loops around the DMA included, for two 32-cycle MFMAs (counters: profiles/r05).
    const int nchunks = p.Kp / 16;
    const int nkt = (p.Kp + KTK - 1) / KTK;
    [[maybe_unused]] const int kt_first = KS ? (int)((long long)ks_part * nkt / p.ks) : 0; // KS: this part's slice of the k-tiles
    const int nit = KS ? (int)((long long)(ks_part + 1) * nkt / p.ks) - kt_first : (nkt + KG - 1) / KG;   // loop trips: KG k-tiles per trip
    const int tchunks = ((nkt + KG - 1) / KG + NSTAGE) * KG * (KTK / 16); // chunks the walk can name (>= nchunks; the tail is dead)
    int *const btab = reinterpret_cast<int *>(smem + NSTAGE * STAGE);
    {
        const int cpc = (RT || p.conv) ? p.Cp / 16 : 1; // chunks per tap
        for (int c = t; c < tchunks; c += 256 * KG) {
            int off = -1; // dead chunk: K padding
            if (c < nchunks) {
                if (RT || p.conv) {
                    const int tap = rten_div(c, p.d_cpc), cc = c - tap * cpc, ky = rten_div(tap, p.d_kw), kx = tap - ky * p.KW;
                    if (ky < p.KH) off = ((cc * p.Hp + ky * p.dy) * p.Wp + kx * p.dx) * 16;
                } else {
                    off = c * 16 * p.N;
                }
            }
            btab[c] = off;
        }
    }
    __syncthreads();
    I8_STAMP(1) // chunk -> offset table in LDS + barrier
    // ---- BQ: DynamicQuantizeLinear parameters from the producer's statistics (every workgroup folds the 256 slots; min / max are
    // order-free), the quantizer's outputs, and this thread's pieces of the B tile
    [[maybe_unused]] float q_scale = 0.f, q_inv = 0.f;
    [[maybe_unused]] int q_zp = 0;
    constexpr int NP = BQ ? 4 * BN / 256 : 1; // 16-byte pieces (16 channels of one pixel) per thread per k-tile
    [[maybe_unused]] unsigned q_voff = OOB;   // byte offset of (image, channel 0, pixel) of this thread's pixel
    [[maybe_unused]] int q_slot0 = 0, q_px = 0;
    if constexpr (BQ || QO == 2) {
        float a = __builtin_inff(), b = -__builtin_inff();
        a = dql::ord2f(p.in_stats[t & 255]);
        b = dql::ord2f(p.in_stats[dql::kStatSlots + (t & 255)]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { a = fminf(a, __shfl_xor(a, o, 64)); b = fmaxf(b, __shfl_xor(b, o, 64)); }
        float *red = reinterpret_cast<float *>(smem + NSTAGE * STAGE + tchunks * 4); // 8 floats behind the chunk table (the launcher sizes the allocation for them)
        if (lane == 0 && wave_all < 4) { red[wave_all] = a; red[4 + wave_all] = b; }
        __syncthreads();
        const float mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3])), mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        const dql::QParams q = dql::dql_params(mn, mx);
        q_scale = q.scale; q_inv = q.inv_scale; q_zp = q.zp;
        if (BQ && t == 0 && blockIdx.x == 0) {
            if (p.xs_out) *p.xs_out = q.scale;
            if (p.xz_out) *p.xz_out = (uint8_t)q.zp;
        }
    }
    if constexpr (BQ) {
        q_px = t % BN;
        q_slot0 = __builtin_amdgcn_readfirstlane(t / BN); // wave-uniform: BN is a multiple of 64
        const int n = n0 + q_px;
        if (n < p.N) {
            const int img = rten_div(n, p.d_hw), pp = n - img * p.HW;
            q_voff = (unsigned)((img * p.Cin) * p.HW + pp) * 4u;
        }
    }
    int ch_idx = __builtin_amdgcn_readfirstlane(wave_all + (KS ? kt_first * (KTK / 16) : 0)); // chunk index of the next piece to issue: wave_all, wave_all + 4 KG, ...
    // the table entries of this wave's next 64 pieces ride in one vector register (lane i = i-th piece from here) and are picked
    // with v_readlane: no LDS round trip on the issue path.  Refilled every 64 pieces.
    auto bo_fill = [&](int first) {
        const int c = first + 4 * KG * lane;
        return c < tchunks ? btab[c] : -1;
    };
    int bo_vec = bo_fill(ch_idx);
    int bo_pos = 0;
    const unsigned a_step = 16u * (unsigned)p.M;
    typedef __attribute__((address_space(3))) void *lds_ptr_t;
    auto issue_tile = [&](int stage) {
#pragma unroll
        for (int q = 0; q < CPW; q++) { // LDS chunk slot wave + 4 q of the tile <- this wave's next chunk (its walk is every 4th chunk)
            uint8_t *As = smem + stage * STAGE + kg * SUB + (wave + 4 * q) * BM * 16;
            uint8_t *Bs = smem + stage * STAGE + kg * SUB + BM * KTK + (wave + 4 * q) * BN * 16;
            const int bo = __builtin_amdgcn_readlane(bo_vec, bo_pos);
            const bool a_live = ch_idx < nchunks, b_live = bo >= 0;
            const unsigned a_soff = a_live ? (unsigned)ch_idx * a_step : 0u;
            const unsigned b_soff = b_live ? (unsigned)bo : 0u;
#pragma unroll
            for (int j = 0; j < RA; j++)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_t)(As + j * 1024), 16, (int)(a_live ? a_voff[j] : OOB), (int)a_soff, 0, 0);
            if constexpr (!BQ) {
#pragma unroll
                for (int j = 0; j < RB; j++)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr_t)(Bs + j * 1024), 16, (int)(b_live ? b_voff[j] : OOB), (int)b_soff, 0, 0);
            }
            ch_idx += 4 * (CPW == 1 ? KG : 1);
            if (++bo_pos == 64) {
                bo_vec = bo_fill(ch_idx);
                bo_pos = 0;
            }
        }
    };

    // BQ: the f32 values of k-tile kt (its 64 channels) for this thread's NP pieces -> registers; later -> codes -> LDS
    [[maybe_unused]] float qv[NP][16];
    [[maybe_unused]] auto q_load = [&](int kt) {
#pragma unroll
        for (int r = 0; r < NP; r++) {
            const int slot = q_slot0 + r * (256 / BN);
            const unsigned soff = (unsigned)((kt * 64 + slot * 16) * p.HW) * 4u; // channel kt*64 + slot*16 (+ j): beyond Cin -> out of range -> 0, never used
#pragma unroll
            for (int j = 0; j < 16; j++)
                qv[r][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsB, (int)q_voff, (int)(soff + (unsigned)(j * p.HW) * 4u), 0));
        }
    };
    [[maybe_unused]] auto q_store = [&](int stage) {
#pragma unroll
        for (int r = 0; r < NP; r++) {
            const int slot = q_slot0 + r * (256 / BN);
            unsigned w[4];
#pragma unroll
            for (int d = 0; d < 4; d++) {
                w[d] = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) w[d] |= ((dql::quant_u8(qv[r][4 * d + j], q_inv, q_zp) ^ 0x80u) & 0xffu) << (8 * j);
            }
            *reinterpret_cast<uint4 *>(smem + stage * STAGE + BM * KTK + (slot * BN + q_px) * 16) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    };

    const int wm0 = (wq / WN) * (BM / WM), wn0 = (wq % WN) * (BN / WN);
    i32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0;
    int cs[TN];
#pragma unroll
    for (int j = 0; j < TN; j++) cs[j] = 0;

    auto compute_tile = [&](int stage) {
        const uint8_t *As = smem + stage * STAGE + kg * SUB + (wm0 + l31) * 16;
        const uint8_t *Bs = smem + stage * STAGE + kg * SUB + BM * KTK + (wn0 + l31) * 16;
        constexpr int NS = KTK / 32; // MFMA k-steps per tile; all fragment reads of a 64-byte tile are issued before its first MFMA
        i32x4 af[NS < 2 ? NS : 2][TM], bf[NS < 2 ? NS : 2][TN];
#pragma unroll
        for (int s0 = 0; s0 < NS; s0 += 2) {
#pragma unroll
            for (int u = 0; u < 2 && s0 + u < NS; u++) {
                const int s = s0 + u;
#pragma unroll
                for (int i = 0; i < TM; i++) af[u][i] = *reinterpret_cast<const i32x4 *>(As + ((2 * s + half) * BM + i * 32) * 16);
#pragma unroll
                for (int j = 0; j < TN; j++) bf[u][j] = *reinterpret_cast<const i32x4 *>(Bs + ((2 * s + half) * BN + j * 32) * 16);
            }
#pragma unroll
            for (int u = 0; u < 2 && s0 + u < NS; u++) {
                if (!RT && p.need_csum) {
#pragma unroll
                    for (int j = 0; j < TN; j++)
#pragma unroll
                        for (int q = 0; q < 4; q++) cs[j] = __builtin_amdgcn_sdot4(bf[u][j][q], 0x01010101, cs[j], false);
                }
#pragma unroll
                for (int i = 0; i < TM; i++)
#pragma unroll
                    for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[u][i], bf[u][j], acc[i][j], 0, 0, 0);
            }
        }
    };

    // ---- epilogue operands, requested BEFORE the main loop so that their latency hides behind it (these short-K
    // products are otherwise epilogue-latency bound): per-row constants by threads 0..BM-1 (parked in LDS once the
    // stage buffers are free), per-column constants and the residual tile straight into registers.  They are older
    // than every LDS-DMA load, so the counted vmcnt waits of the main loop cover them.
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void *)p.C, 0, 0x7ffffffc, 0x00020000);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc((void *)(p.res ? (const void *)p.res : (const void *)p.C), 0, 0x7ffffffc, 0x00020000);
    const unsigned rs4 = (unsigned)p.c_rs << 2;
    const int mb = m0 + wm0 + 4 * half;
    int rc_rsum = 0, rc_az_raw = -1;
    float rc_bias = 0.f, rc_srow = 0.f;
    if (t < BM) { // (threads of k-group 0)
        const int m = m0 + t < p.M ? m0 + t : 0;
        rc_rsum = p.rsum[m];
        if constexpr (!RT) rc_az_raw = zp_raw(p.a_zp, p.a_zp_len > 1 ? m % p.a_zp_len : 0); // GEMM: period < M cycles the zero points (matmul.rs:266-280)
        rc_bias = p.bias ? p.bias[m] : 0.f;
        rc_srow = (p.scale && p.scale_per_row) ? p.scale[m] : 0.f;
        if constexpr (BQ) rc_srow = q_scale * rc_srow; // Mul(x_scale, w_scale[m])
    }
    unsigned basev[TN], bzv[TN], csv[TN];
    [[maybe_unused]] int bz_raw[TN]; // (converted after the main loop: zp_from_raw)
    // RT: ONE activation zero point for the whole launch.  A wave-uniform byte load comes back through a vector register and v_readfirstlane, i.e. with a
    // full drain of the vector-memory counter right here; the aligned word around the byte through the scalar cache instead is only waited for where it is used.
    [[maybe_unused]] unsigned bz_word = 0;
    [[maybe_unused]] int bz_shift = -1;
    if constexpr (RT && !BQ) {
        if (p.b_zp) {
            const unsigned long long addr = (unsigned long long)p.b_zp;
            bz_word = *(const __attribute__((address_space(4))) unsigned *)(addr & ~3ull);
            bz_shift = (int)(addr & 3ull) * 8;
        }
    }
    float scv[TN];
#pragma unroll
    for (int j = 0; j < TN; j++) {
        const int n = n0 + wn0 + j * 32 + l31;
        const bool cok = n < p.N;
        const int nn = cok ? n : 0;
        const int nb = rten_div(nn, p.d_pn), np = nn - nb * p.Pn;
        basev[j] = cok ? (unsigned)((long long)nb * p.c_ns + np) << 2 : OOB; // byte offset of (row 0, column n); rows ride the scalar offset
        if constexpr (!RT) bz_raw[j] = zp_raw(p.b_zp, p.b_zp_len == 1 ? 0 : nn);
        bzv[j] = 0u;
        csv[j] = (!RT && p.csum) ? (unsigned)p.csum[nn] : 0u;
        scv[j] = (p.scale && !p.scale_per_row) ? p.scale[p.scale_len == 1 ? 0 : nn] : 0.f;
        if constexpr (BQ) {
            bzv[j] = (unsigned)(q_zp - 128);   // the activation zero point in the signed domain
            scv[j] = q_scale * scv[j];         // Mul(x_scale, w_scale)
        }
    }
    // row r of 32-row block i sits at scalar byte offset (mb_u + i*32 + acc_row(r)) * rs4, with mb_u wave-uniform and the lane's
    // half (rows +4) folded into the vector offset
    const unsigned half_off = (unsigned)(4 * half) * rs4;
    const int mb_u = m0 + (wave / WN) * (BM / WM);
    I8_STAMP(2) // quantizer parameters (BQ), zero points / scales / row constants of this lane's columns and rows
    [[maybe_unused]] float rr[RES ? TM : 1][RES ? TN : 1][16];
    if constexpr (RES) {
        if (KG == 1 || kg == 0) {
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < TN; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int m = mb + i * 32 + acc_row(r);
                        const unsigned vo = (m < p.M && basev[j] != OOB) ? basev[j] + half_off : OOB;
                        rr[i][j][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsR, (int)vo, (int)((unsigned)(mb_u + i * 32 + acc_row(r)) * rs4), 0));
                    }
        }
    }

    I8_STAMP(3) // residual tile requested (RES)
    int stage = 0;
    if constexpr (BQ) {
        // A by DMA two tiles ahead (as below); B: the values of tile it + 1 are in flight in registers while tile it is multiplied,
        // and are converted and written to their stage at the top of the next trip, before the barrier that publishes it.
#pragma unroll
        for (int i = 0; i < NSTAGE - 1; i++) issue_tile(i);
        q_load(0);
        wait_vmcnt<0>();
        q_store(0);
        q_load(1);
        I8_STAMP(4) // first operand tiles requested (and the first B tile converted)
        for (int it = 0; it < nit; it++) {
            wait_vmcnt<0>(); // A of tile it (and it + 1), B values of tile it + 1
            const int stn = stage == NSTAGE - 1 ? 0 : stage + 1;
            q_store(stn);    // stage of tile it + 1: last read two trips ago
            __builtin_amdgcn_s_barrier();
            const int stp = stage == 0 ? NSTAGE - 1 : stage - 1;
            issue_tile(stp); // A of tile it + 2
            q_load(it + 2);
            compute_tile(stage);
            stage = stn;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NSTAGE - 1; i++) issue_tile(i);
        // (A two-fragment-set software pipeline of the LDS reads under the MFMAs was measured and is slower.)
        I8_STAMP(4) // first operand tiles requested
        for (int it = 0; it < nit; it++) {
            wait_vmcnt<PER_TILE *(NSTAGE - 2)>();
            __builtin_amdgcn_s_barrier();
            const int stp = stage == 0 ? NSTAGE - 1 : stage - 1;
            issue_tile(stp);
            compute_tile(stage);
            stage = stage == NSTAGE - 1 ? 0 : stage + 1;
        }
    }
    I8_STAMP(5) // k-loop
    wait_vmcnt<0>();
    __syncthreads(); // every wave is done with the stage buffers
    if constexpr (KS) {
        constexpr int NQ = TM * TN * 4; // 16-byte pieces per lane
        const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc((void *)(p.slab + ((long long)tile * p.ks) * (BM * BN)), 0, (int)((unsigned)p.ks * (BM * BN) * 4u), 0x00020000);
        const unsigned lane_off = (unsigned)(wave * (NQ * 64) + lane) * 16u;
        const unsigned part_bytes = (unsigned)(BM * BN) * 4u;
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) // aux 17 = sc0 sc1: the store writes through to memory (the eight XCD L2s are not coherent with each other inside a kernel)
                    __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{(unsigned)acc[i][j][4 * q], (unsigned)acc[i][j][4 * q + 1], (unsigned)acc[i][j][4 * q + 2], (unsigned)acc[i][j][4 * q + 3]},
                                                           rsS, (int)(lane_off + (unsigned)(((i * TN + j) * 4 + q) * 64) * 16u), (int)((unsigned)ks_part * part_bytes), 17);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's write-through stores are acknowledged
        __syncthreads();
        int *const flag = reinterpret_cast<int *>(smem);
        if (t == 0) {
            const unsigned old = __hip_atomic_fetch_add(p.ks_counters + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *flag = old == (unsigned)p.ks - 1u;
        }
        __syncthreads();
        const bool last = *flag != 0;
        __syncthreads(); // (the row constants are parked over the same LDS bytes next)
        if (!last) return;
        for (int q2 = 0; q2 < p.ks; q2++) {
            if (q2 == ks_part) continue;
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < TN; j++)
#pragma unroll
                    for (int q = 0; q < 4; q++) { // L2-bypassing loads: the other parts were written by workgroups on any XCD
                        const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rsS, (int)(lane_off + (unsigned)(((i * TN + j) * 4 + q) * 64) * 16u), (int)((unsigned)q2 * part_bytes), 17);
                        acc[i][j][4 * q] += (int)v[0]; acc[i][j][4 * q + 1] += (int)v[1]; acc[i][j][4 * q + 2] += (int)v[2]; acc[i][j][4 * q + 3] += (int)v[3];
                    }
        }
        if (t == 0) p.ks_counters[tile] = 0u; // every launch leaves its counters zero
    }
    if constexpr (KG > 1) {
        // partial sums of k-groups 1 .. KG-1 -> LDS ([group][register][thread of the group]: 1 KiB per wave store), added by group 0
        int *red = reinterpret_cast<int *>(smem);
        constexpr int RW = TM * TN * 16 + TN; // words per thread: accumulators + column-sum partials
        const int tg = t & 255;
        if (kg > 0) {
            int *dst = red + (kg - 1) * RW * 256 + tg;
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < TN; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) dst[((i * TN + j) * 16 + r) * 256] = acc[i][j][r];
            if constexpr (!RT) {
#pragma unroll
                for (int j = 0; j < TN; j++) dst[(TM * TN * 16 + j) * 256] = cs[j];
            }
        }
        __syncthreads();
        if (kg == 0) {
#pragma unroll
            for (int g = 1; g < KG; g++) {
                const int *src = red + (g - 1) * RW * 256 + tg;
#pragma unroll
                for (int i = 0; i < TM; i++)
#pragma unroll
                    for (int j = 0; j < TN; j++)
#pragma unroll
                        for (int r = 0; r < 16; r++) acc[i][j][r] += src[((i * TN + j) * 16 + r) * 256];
                if constexpr (!RT) {
#pragma unroll
                    for (int j = 0; j < TN; j++) cs[j] += src[(TM * TN * 16 + j) * 256];
                }
            }
        }
        __syncthreads(); // the row constants are parked over the same bytes next
    }
    int *rowc = reinterpret_cast<int *>(smem); // [4][BM]: row sum, a_zp, bias, per-row scale
    if (t < BM) {
        rowc[t] = rc_rsum;
        if constexpr (!RT) rowc[BM + t] = zp_from_raw(rc_az_raw, p.a_signed);
        rowc[2 * BM + t] = __builtin_bit_cast(int, rc_bias);
        rowc[3 * BM + t] = __builtin_bit_cast(int, rc_srow);
    }
    __syncthreads();
    if (!RT && !p.csum) {
#pragma unroll
        for (int j = 0; j < TN; j++) csv[j] = (unsigned)(cs[j] + __shfl_xor(cs[j], 32, 64)); // the two k halves of the column
    }
    I8_STAMP(6) // drain, k-group reduction, row constants through LDS
    if constexpr (!BQ) {
        [[maybe_unused]] const int raw_u = bz_shift < 0 ? -1 : (int)((bz_word >> bz_shift) & 0xffu);
#pragma unroll
        for (int j = 0; j < TN; j++) bzv[j] = (unsigned)zp_from_raw(RT ? raw_u : bz_raw[j], p.b_signed);
    }
    const bool epi = KG == 1 || kg == 0; // the epilogue belongs to k-group 0
    if (QO != 1 && !epi) return;         // (no barrier follows; the grid-wide exchange of QO == 1 needs every wave of the workgroup)

    // ---- epilogue: zero-point algebra, optional cast_scale / bias / residual / relu, store.  16 accumulator
    // registers (one 32 x 32 block) are finished at a time; all of a block's stores are issued back to back.
    float st_mn = __builtin_inff(), st_mx = -__builtin_inff(); // output statistics for the consuming DynamicQuantizeLinear
    const int ml0 = wm0 + 4 * half;
    const bool full_rows = m0 + BM <= p.M;                                                           // (workgroup-uniform)
    constexpr bool rowterm_only = RT; // weight zero point 0, one activation zero point (the launcher checks: a_zp == NULL, signed A, b_zp_len <= 1)
    if (epi) {
#pragma unroll
    for (int i = 0; i < TM; i++) {
        unsigned rsv[16], azv[16];
        float bv[16], srow[16];
        bool mok[16];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int ml = ml0 + i * 32 + acc_row(r);
            mok[r] = m0 + ml < p.M;
            rsv[r] = (unsigned)rowc[ml];
            azv[r] = RT ? 0u : (unsigned)rowc[BM + ml];
            bv[r] = __builtin_bit_cast(float, rowc[2 * BM + ml]);
            srow[r] = __builtin_bit_cast(float, rowc[3 * BM + ml]);
        }
        // The convolution form of every ort-quantized graph -- weight zero point 0 (signed weights without a zero-point input), ONE activation
        // zero point -- needs a single correction term per ROW, bz * rowsum(A): formed once per 32-row block instead of three multiplies and
        // three adds per element (the epilogue of these short-K launches is VALU-issue bound: tools/debug/i8_trace.py measured 2.7-5.4 us of
        // epilogue next to a 2-7 us k-loop).  Same integers: the dropped terms are multiplied by a zero.
        [[maybe_unused]] unsigned trow[16];
        if constexpr (rowterm_only) {
#pragma unroll
            for (int r = 0; r < 16; r++) trow[r] = bzv[0] * rsv[r];
        }
#pragma unroll
        for (int j = 0; j < TN; j++) {
            const bool cok = basev[j] != OOB;
            unsigned v[16];
            if constexpr (rowterm_only) {
#pragma unroll
                for (int r = 0; r < 16; r++) v[r] = (unsigned)acc[i][j][r] - trow[r];
            } else {
#pragma unroll
                for (int r = 0; r < 16; r++)
                    v[r] = (unsigned)acc[i][j][r] - bzv[j] * rsv[r] - azv[r] * csv[j] + (unsigned)p.Kreal * azv[r] * bzv[j];
            }
            if (p.scale) {
                float f[16];
                if (p.scale_per_row) {
#pragma unroll
                    for (int r = 0; r < 16; r++) f[r] = (float)(int)v[r] * srow[r]; // cast_scale (matmul.rs:751,761)
                } else {
                    const float sj = scv[j];
#pragma unroll
                    for (int r = 0; r < 16; r++) f[r] = (float)(int)v[r] * sj;
                }
                if (p.bias) {
#pragma unroll
                    for (int r = 0; r < 16; r++) f[r] = f[r] + bv[r];
                }
                if constexpr (RES) {
#pragma unroll
                    for (int r = 0; r < 16; r++) f[r] = f[r] + rr[i][j][r];
                }
                if (p.relu) {
#pragma unroll
                    for (int r = 0; r < 16; r++) f[r] = vm::relu(f[r]);
                }
                if (p.stats) { // fminf / fmaxf drop NaNs like the reference's min/max sweep (min_max.rs:27-30)
                    if (full_rows) { // every row of the tile exists: one column test for the block
                        if (cok) {
#pragma unroll
                            for (int r = 0; r < 16; r++) { st_mn = fminf(f[r], st_mn); st_mx = fmaxf(f[r], st_mx); }
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; r++)
                            if (mok[r] && cok) { st_mn = fminf(f[r], st_mn); st_mx = fmaxf(f[r], st_mx); }
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; r++) v[r] = __builtin_bit_cast(unsigned, f[r]);
            }
            if constexpr (QO) { // the finished values wait in the accumulator registers for the grid-wide statistics
#pragma unroll
                for (int r = 0; r < 16; r++) acc[i][j][r] = (int)v[r];
            }
            if ((!QO || p.C) && !p.no_store) {
                const unsigned vo_col = cok ? basev[j] + half_off : OOB;
                if (full_rows) {
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        __builtin_amdgcn_raw_buffer_store_b32(v[r], rsC, (int)vo_col, (int)((unsigned)(mb_u + i * 32 + acc_row(r)) * rs4), 0);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        __builtin_amdgcn_raw_buffer_store_b32(v[r], rsC, (int)(mok[r] ? vo_col : OOB), (int)((unsigned)(mb_u + i * 32 + acc_row(r)) * rs4), 0);
                }
            }
        }
    }
    } // epi
    if constexpr (QO != 0) {
        dql::QParams q;
        const unsigned G = gridDim.x;
        if constexpr (QO == 2) { // the statistics came from the previous launch (folded in the prologue): straight to the codes
            q.scale = q_scale; q.inv_scale = q_inv; q.zp = q_zp;
            if (t == 0 && blockIdx.x == 0) {
                *p.q_scale_out = q.scale;
                *p.q_zp_out = (uint8_t)q.zp;
                if (p.q_mul_by) *p.q_product = q.scale * p.q_mul_by[0];
            }
        } else {
        // ---- (1) all-gather of the workgroups' min / max.  One hop: every workgroup publishes ONE 8-byte granule {min, max} (ordered-uint
        // images; the pair a reset leaves there, {0xffffffff, 0}, cannot be a real one, so the data is its own flag) with a write-through
        // store and then sweeps all G granules with relaxed agent-scope loads until none is the reset pair.  No counters, no fences, no
        // read-modify-write on the critical path (the first version -- eight arrival counters polled by every workgroup plus the slot
        // atomics -- cost 6 / 9 / 22 us at 200 / 392 / 784 workgroups: profiles/r06/int8_qout_per_layer.txt).
        unsigned long long *const gran = reinterpret_cast<unsigned long long *>(p.sync + kSyncCtlWords);
        float *const gred = reinterpret_cast<float *>(smem + 8192); // (the row constants at the start of the stage buffers are dead by now)
        if (epi) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) { st_mn = fminf(st_mn, __shfl_xor(st_mn, o, 64)); st_mx = fmaxf(st_mx, __shfl_xor(st_mx, o, 64)); }
            if (lane == 0) {
                gred[wq] = st_mn; gred[4 + wq] = st_mx;
                // the statistics block as rten_hip_conv2d_int8_stats leaves it (for a second reader of the f32 output); nobody waits for these
                const unsigned slot = (blockIdx.x * 4u + (unsigned)wq) % (unsigned)dql::kStatSlots;
                atomicMin(&p.stats[slot], dql::f2ord(st_mn));
                atomicMax(&p.stats[dql::kStatSlots + slot], dql::f2ord(st_mx));
            }
        }
        __syncthreads();
        if (t == 0) {
            const float mn = fminf(fminf(gred[0], gred[1]), fminf(gred[2], gred[3])), mx = fmaxf(fmaxf(gred[4], gred[5]), fmaxf(gred[6], gred[7]));
            __hip_atomic_store(gran + blockIdx.x, ((unsigned long long)dql::f2ord(mx) << 32) | dql::f2ord(mn), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        float ga = __builtin_inff(), gb = -__builtin_inff();
        for (unsigned spins = 0;;) {
            bool ok = true;
            ga = __builtin_inff(); gb = -__builtin_inff();
            for (unsigned g = (unsigned)t; g < G; g += 256u * KG) {
                const unsigned long long v = __hip_atomic_load(gran + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = ok && v != kGranuleReset;
                ga = fminf(ga, dql::ord2f((unsigned)v)); gb = fmaxf(gb, dql::ord2f((unsigned)(v >> 32)));
            }
            if (__syncthreads_and(ok)) break;
            if (++spins >= kSyncSpinLimit) { // not every workgroup is resident (or a previous launch timed out): give up, LOUDLY --
                // the block's time-out flag, the context's sticky fault word (the next rten_hip_sync / graph_launch fails) and a NaN scale for the
                // consumer (below): statistics that miss a workgroup must never turn into plausible codes
                if (t == 0) {
                    __hip_atomic_store(p.sync + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (p.fault) __hip_atomic_store(p.fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    *p.q_scale_out = __builtin_nanf("");
                    if (p.q_mul_by) *p.q_product = __builtin_nanf("");
                }
                break;
            }
            __builtin_amdgcn_s_sleep(4);
        }
        if (t == 0) { // the last workgroup out resets the granules for the next launch (everybody has finished sweeping by then)
            const unsigned old = __hip_atomic_fetch_add(p.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            gred[8] = old == G - 1u ? 1.f : 0.f;
        }
        // ---- (2) the statistics of the whole tensor -> DynamicQuantizeLinear's parameters (quantize.rs:397-419)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { ga = fminf(ga, __shfl_xor(ga, o, 64)); gb = fmaxf(gb, __shfl_xor(gb, o, 64)); }
        if (lane == 0) { gred[16 + wave_all] = ga; gred[32 + wave_all] = gb; }
        __syncthreads();
        if (gred[8] != 0.f) {
            for (unsigned g = (unsigned)t; g < G; g += 256u * KG) __hip_atomic_store(gran + g, kGranuleReset, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t == 0) __hip_atomic_store(p.sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!epi) return;
        float g_mn = gred[16], g_mx = gred[32];
#pragma unroll
        for (int wv = 1; wv < 4 * KG; wv++) { g_mn = fminf(g_mn, gred[16 + wv]); g_mx = fmaxf(g_mx, gred[32 + wv]); }
        q = dql::dql_params(g_mn, g_mx);
        if (t == 0 && blockIdx.x == 0) {
            // (a workgroup that timed out -- before or after this store -- leaves NaN here: whoever gives up first has set the flag)
            const bool void_run = __hip_atomic_load(p.sync + 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
            *p.q_scale_out = void_run ? __builtin_nanf("") : q.scale;
            *p.q_zp_out = (uint8_t)q.zp;
            if (p.q_mul_by) *p.q_product = void_run ? __builtin_nanf("") : q.scale * p.q_mul_by[0]; // the Mul(x_scale, w_scale) node of the consumer
        }
        } // QO == 1
        // ---- (3) codes -> the consumer's staged image [N][C/16][Hp][Wp][16 B] (signed domain).  A lane holds, per 32-row block, four
        // dwords of four consecutive channels each: rows 0-3, 8-11, 16-19, 24-27 (+4 in the upper half of the wave); two
        // v_permlane32_swap give the lower half the sixteen channels 0-15 of its pixel and the upper half channels 16-31.
        const __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc((void *)p.q_out, 0, (int)p.q_bytes, 0x00020000);
#pragma unroll
        for (int j = 0; j < TN; j++) {
            const int n = n0 + wn0 + j * 32 + l31;
            const bool cok = n < p.N;
            const int nn = cok ? n : 0;
            const int nb = rten_div(nn, p.d_pn), np = nn - nb * p.Pn;
            const int oy = rten_div(np, p.d_qw), ox = np - oy * p.q_W;
            const unsigned pix = (unsigned)((oy + p.q_pt) * p.q_Wp + ox + p.q_pl);
#pragma unroll
            for (int i = 0; i < TM; i++) {
                unsigned d[4];
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    d[g] = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const int bits = acc[i][j][4 * g + b]; // (copied to a scalar first: a bit_cast applied directly to an ext-vector element reads element 0 under this compiler)
                        d[g] |= ((dql::quant_u8(__int_as_float(bits), q.inv_scale, q.zp) ^ 0x80u) & 0xffu) << (8 * b);
                    }
                }
                const auto s02 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false); // {lower: own d0 | upper: partner's d2}, {partner's d0 | own d2}
                const auto s13 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                const unsigned w0 = s02[0], w1 = s02[1], w2 = s13[0], w3 = s13[1];
                const int chunk = (m0 + wm0 + i * 32) / 16 + half;
                const unsigned off = (chunk * 16 < p.M && cok) ? ((unsigned)((nb * p.q_cb + chunk) * (p.q_Hp * p.q_Wp)) + pix) * 16u : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{w0, w1, w2, w3}, rsQ, (int)off, 0, 0);
            }
        }
        // border pieces of the consumer's padding (value of its pad mode), dealt over the whole grid
        const int nbp = p.q_Hp * p.q_Wp - p.q_H * p.q_W;
        if (nbp > 0) {
            int pad_s = 0;
            if (p.q_pad_mode == RTEN_HIP_PAD_ZERO_POINT) pad_s = q.zp - 128;
            else if (p.q_pad_mode == RTEN_HIP_PAD_RAW0_U8) pad_s = -128;
            const unsigned fb = ((unsigned)pad_s & 0xffu) * 0x01010101u;
            const int planes = (p.N / p.Pn) * p.q_cb, total = planes * nbp;
            const int top = p.q_pt * p.q_Wp, side = p.q_Wp - p.q_W;
            for (int idx = (int)blockIdx.x * 256 + t; idx < total; idx += (int)G * 256) {
                const int plane = idx / nbp, b = idx - plane * nbp;
                int pos;
                if (b < top) pos = b;
                else {
                    const int b1 = b - top;
                    if (side > 0 && b1 < p.q_H * side) {
                        const int row = b1 / side, wi = b1 - row * side;
                        pos = (p.q_pt + row) * p.q_Wp + (wi < p.q_pl ? wi : p.q_W + wi);
                    } else pos = (p.q_pt + p.q_H) * p.q_Wp + (b1 - p.q_H * side);
                }
                __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{fb, fb, fb, fb}, rsQ, (int)(((unsigned)(plane * (p.q_Hp * p.q_Wp)) + (unsigned)pos) * 16u), 0, 0);
            }
        }
#ifdef RTEN_TRACE
        {
            I8_STAMP(7) // epilogue (zero-point algebra, scale, bias, residual, statistics, stores issued; QO: + the grid-wide exchange and the quantized stores)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned long long t_end_ = __builtin_readcyclecounter();
            if (blockIdx.x == (gridDim.x > 8 ? 8 : 0) && t == 0)
                printf("[i8 trace] <%d,%d,res=%d,kg=%d,bq=%d,qo=%d,rt=%d> M %d N %d Kp %d grid %u: args+decode %llu, table %llu, operands %llu, residual req %llu, first tiles %llu, k-loop %llu (%d trips), drain+rowc %llu, epilogue %llu, store drain %llu cycles\n",
                       BM, BN, (int)RES, KG, (int)BQ, (int)QO, (int)RT, p.M, p.N, p.Kp, gridDim.x, tr_seg[0], tr_seg[1], tr_seg[2], tr_seg[3], tr_seg[4], tr_seg[5], nit, tr_seg[6], tr_seg[7], t_end_ - tr_prev);
        }
#endif
        return;
    }
    if (p.stats) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { st_mn = fminf(st_mn, __shfl_xor(st_mn, o, 64)); st_mx = fmaxf(st_mx, __shfl_xor(st_mx, o, 64)); }
        if (lane == 0) {
            const unsigned slot = (blockIdx.x * 4u + (unsigned)wq) % (unsigned)dql::kStatSlots;
            atomicMin(&p.stats[slot], dql::f2ord(st_mn));
            atomicMax(&p.stats[dql::kStatSlots + slot], dql::f2ord(st_mx));
        }
    }
#ifdef RTEN_TRACE
    {
        I8_STAMP(7) // epilogue (zero-point algebra, scale, bias, residual, statistics, stores issued; QO: + the grid-wide exchange and the quantized stores)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long t_end_ = __builtin_readcyclecounter();
        if ((blockIdx.x == (gridDim.x > 8 ? 8 : 0) || (gridDim.x > 64 && blockIdx.x == gridDim.x - 9)) && t == 0) // (an early workgroup and a late one)
            printf("[i8 trace] <%d,%d,res=%d,kg=%d,bq=%d,qo=%d,rt=%d> M %d N %d Kp %d grid %u: args+decode %llu, table %llu, operands %llu, residual req %llu, first tiles %llu, k-loop %llu (%d trips), drain+rowc %llu, epilogue %llu, store drain %llu cycles; %llu cycles in %llu ticks of 10 ns\n",
                   BM, BN, (int)RES, KG, (int)BQ, (int)QO, (int)RT, p.M, p.N, p.Kp, gridDim.x, tr_seg[0], tr_seg[1], tr_seg[2], tr_seg[3], tr_seg[4], tr_seg[5], nit, tr_seg[6], tr_seg[7], t_end_ - tr_prev,
                   t_end_ - tr_c0, (unsigned long long)__builtin_amdgcn_s_memrealtime() - tr_r0);
    }
#endif
#undef I8_STAMP
}

// Workgroups of `kern` (threads, dynamic LDS) the whole device holds at once (the occupancy query is cached per kernel and LDS size).
int resident_capacity(rten_hip_ctx *ctx, const void *kern, int threads, size_t lds) {
    static std::mutex mu;
    static std::map<std::pair<const void *, size_t>, int> cache;
    std::lock_guard<std::mutex> g(mu);
    const auto key = std::make_pair(kern, lds);
    auto it = cache.find(key);
    if (it == cache.end()) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, lds) != hipSuccess) nb = 0;
        it = cache.emplace(key, nb < 8 ? nb : 8).first;
    }
    return it->second * ctx->num_cus;
}

enum Form { PLAIN, LOADQ /* BQ */, EXCHANGE /* QO == 1 */, RECOMPUTE /* QO == 2 */, KSPLIT /* KS */, kForms }; // the launch forms ...
enum Tile { T128x128, T128x64, T64x128, T64x64, T64x64_KG4, T64x256, kTiles, kNoTile = kTiles }; // ... and the tiles they are launched on
constexpr int kTileM[kTiles] = {128, 128, 64, 64, 64, 64}, kTileN[kTiles] = {128, 64, 128, 64, 64, 256}, kTileKG[kTiles] = {1, 1, 1, 1, 4, 1};

// The name a launch is profiled under: "igemm_i8_fast_kernel<BM,BN[,kg4][,form]>" (plans, tools and tests match on it)
const char *fast_label(Form f, Tile t) {
    static const auto labels = [] {
        const char *const tile[kTiles] = {"128,128", "128,64", "64,128", "64,64", "64,64,kg4", "64,256"};
        const char *const form[kForms] = {"", ",bq", ",qo", ",qo2", ",ks"};
        std::array<std::array<std::string, kTiles>, kForms> l;
        for (int i = 0; i < kForms; i++)
            for (int j = 0; j < kTiles; j++) l[i][j] = std::string("igemm_i8_fast_kernel<") + tile[j] + form[i] + ">";
        return l;
    }();
    return labels[f][t].c_str();
}

// One launch of form F on tile T.  false (nothing launched): an exchange grid that cannot be resident all at once, or a recompute launch outside its form.
// (256-byte k-tiles were measured and are slower: profiles/r05/int8_notes.md.  Measured again in round 3 and dropped -- profiles/r06/int8_tile_experiments.txt:
// 128-byte k-tiles on the smaller tiles +5 % on the whole conv time, the next larger tile for the under-filled launches +6 %, four LDS stages +2 %)
template <Form F, Tile T>
bool launch_fast(rten_hip_ctx *ctx, FastArgs &a, double ops, double bytes) {
    constexpr int BM = kTileM[T], BN = kTileN[T], KG = kTileKG[T], NST = 3, KTK = 64;
    constexpr bool BQ = F == LOADQ, KS = F == KSPLIT;
    constexpr int QO = F == EXCHANGE ? 1 : F == RECOMPUTE ? 2 : 0;
    a.tiles_m = (a.M + BM - 1) / BM;
    a.tiles_n = (a.N + BN - 1) / BN;
    constexpr size_t ring = (size_t)NST * KG * (BM + BN) * KTK;
    static_assert(ring <= 128 * 1024, "int8 tile ring exceeds the LDS of a compute unit");
    const int nkt = (a.Kp + KTK - 1) / KTK;
    const size_t lds = ring + (size_t)((nkt + KG - 1) / KG + NST) * KG * (KTK / 16) * 4 + 64; // + the chunk -> B offset table + the statistics fold's scratch
    a.d_pn = rten_make_div((long long)a.tiles_n * BN, a.Pn);
    a.d_tile = rten_make_div((long long)a.tiles_m * a.tiles_n, a.n_fastest ? a.tiles_n : a.tiles_m);
    if (BQ) a.d_hw = rten_make_div((long long)a.tiles_n * BN, a.HW);
    if (QO) a.d_qw = rten_make_div(a.Pn, a.q_W);
    if (a.conv) {
        const long long tchunks = (long long)((nkt + KG - 1) / KG + NST) * KG * (KTK / 16);
        a.d_ow = rten_make_div(a.Pn, a.OW);
        a.d_cpc = rten_make_div(tchunks, a.Cp / 16);
        a.d_kw = rten_make_div(tchunks, a.KW);
    }
    bool launched = true;
    auto go = [&](auto kern) {
        if (lds > 64 * 1024) hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (QO == 1 && ((long long)a.tiles_m * a.tiles_n > resident_capacity(ctx, (const void *)kern, 256 * KG, lds) || (long long)a.tiles_m * a.tiles_n > (long long)kSyncGranules)) {
            launched = false;
            return;
        }
        ProfScope ps(ctx, fast_label(F, T), ops, bytes);
        hipLaunchKernelGGL(kern, dim3((unsigned)(a.tiles_m * a.tiles_n * (KS ? a.ks : 1))), dim3(256 * KG), lds, ctx->stream, a);
    };
    const bool rt = single_row_term(a);
    // (statements, not an `else`, follow the two early-return forms: the RES x RT kernels of their tile are compiled for them too and never launched -- for
    // K split they are the plain form's own, for the recompute form they belong to the library's kernel set as it stands)
    if constexpr (QO == 2) { // the recompute form is built for the single-row-term convolution without a residual (the single-consumer edges of a bottleneck block)
        if (!rt || (a.res && a.scale)) { launched = false; return launched; }
        go(igemm_i8_fast_kernel<BM, BN, NST, false, KTK, KG, BQ, 2, true>);
        return launched;
    }
    if constexpr (KS) { // (the dispatcher checked: RT form, no residual)
        go(igemm_i8_fast_kernel<BM, BN, NST, false, KTK, KG, BQ, QO, true, true>);
        return launched;
    }
    if (rt) {
        if (a.res && a.scale) go(igemm_i8_fast_kernel<BM, BN, NST, true, KTK, KG, BQ, QO, true>);
        else go(igemm_i8_fast_kernel<BM, BN, NST, false, KTK, KG, BQ, QO, true>);
    } else {
        if (a.res && a.scale) go(igemm_i8_fast_kernel<BM, BN, NST, true, KTK, KG, BQ, QO, false>);
        else go(igemm_i8_fast_kernel<BM, BN, NST, false, KTK, KG, BQ, QO, false>);
    }
    return launched;
}

// The tile switch of every form.  A form is compiled for the tiles it has always had: 64x256 for the exchange form only, four k-groups for the forms that take
// the plain tile choice, no 64x128 for K split.  false: nothing launched (launch_fast), or a tile the form is not built for -- which no caller below asks for.
template <Form F>
bool launch_tile(rten_hip_ctx *ctx, FastArgs &a, Tile t, double ops, double bytes) {
    switch (t) {
    case T128x128: return launch_fast<F, T128x128>(ctx, a, ops, bytes);
    case T128x64: return launch_fast<F, T128x64>(ctx, a, ops, bytes);
    case T64x64: return launch_fast<F, T64x64>(ctx, a, ops, bytes);
    case T64x128: if constexpr (F != KSPLIT) return launch_fast<F, T64x128>(ctx, a, ops, bytes); else break;
    case T64x64_KG4: if constexpr (F == PLAIN || F == EXCHANGE || F == RECOMPUTE) return launch_fast<F, T64x64_KG4>(ctx, a, ops, bytes); else break;
    case T64x256: if constexpr (F == EXCHANGE) return launch_fast<F, T64x256>(ctx, a, ops, bytes); else break;
    default: break;
    }
    return false;
}

// tile setting (0 = 128x128, 1 = 128x64, 2 = 64x128, anything else = 64x64) -> tile; `kg4`: the 64x64 tile with four k-groups
Tile tile_of(int setting, bool kg4) { return setting == 0 ? T128x128 : setting == 1 ? T128x64 : setting == 2 ? T64x128 : kg4 ? T64x64_KG4 : T64x64; }
// the next larger tile an exchange launch tries when its grid does not fit the chip at once
Tile next_larger(Tile t) { return t == T128x64 ? T128x128 : t == T64x128 ? T64x256 : t == T64x64 ? T128x64 : kNoTile; }
long long tile_count(const FastArgs &a, Tile t) { return (long long)((a.M + kTileM[t] - 1) / kTileM[t]) * ((a.N + kTileN[t] - 1) / kTileN[t]); }

// K-group rule: under-filled launches (fewer than ~2 workgroups per CU) of the 64x64 tile split K over 4 k-groups inside the workgroup: more waves per SIMD to
// hide the k-loop's latencies behind each other (RTEN_HIP_DEBUG bit 0x800 turns this off).  Measured (profiles/r05/int8_per_layer.txt): 4 groups pay off below
// ~1.25 workgroups per CU with K >= 1024 bytes (stage-4 3x3: 20.8 -> 14.8 us); 2 groups on the 1.5-workgroup launches of stage 3 do not (10.3 -> 11.5 us)
bool four_k_groups(const rten_hip_ctx *ctx, const FastArgs &a) { return !(ctx->debug & 0x800) && tile_count(a, T64x64) * 4 <= 5 * ctx->num_cus && (a.Kp + 63) / 64 >= 16; }

// Cross-workgroup K split (KS kernels): under-filled long-K launches of the single-row-term convolution form without a residual.  `a.ks` = the largest
// split the caller's slab holds (0: none); RTEN_I8_KS = "<parts>[,<tile>]" selects it (a measurement knob: tile 0 = 128x128, 1 = 128x64, else 64x64).
// Returns the tile to split on, with a.ks = the parts; or kNoTile, with a.ks = 0.
Tile k_split_tile(const rten_hip_ctx *ctx, FastArgs &a) {
    static const char *env_ks = getenv("RTEN_I8_KS");
    static const int env_parts = env_ks ? atoi(env_ks) : -1, env_kst = (env_ks && strchr(env_ks, ',')) ? atoi(strchr(env_ks, ',') + 1) : -1;
    int parts = 0;
    if (single_row_term(a) && !a.res && a.ks >= 2 && a.slab && a.ks_counters && !(ctx->debug & 0x1000)) {
        // MEASURED AND NOT USED BY DEFAULT (profiles/r09/int8_cross_workgroup_k_split.txt): every split loses -- s2 3x3 13.7 -> 17.1 us (2 parts, 64x64),
        // 16.9 (2 parts, 128x64), 19.0 (128x128), 20.8 (4 parts); s3 3x3 12.6 -> 15.7; K = 1024 1x1 9.1 -> 13.6; the int8 step 1.48 -> 1.53 ms (one
        // replica), 0.89 -> 0.97 (four).  The hand-off (16-64 KB of write-through partials per workgroup, the counter, the L2-bypassing reload) costs 4-7 us
        // against a k-loop of ~6 us that it can shorten by half at best; the in-workgroup form (k-groups through LDS) stays the rule for stage 3.
        if (env_parts >= 0) parts = env_parts;
        if (parts > a.ks) parts = a.ks;
        if (parts > (a.Kp + 63) / 64) parts = (a.Kp + 63) / 64;
    }
    const Tile t = tile_of(env_kst == 0 || env_kst == 1 ? env_kst : 3, false);
    a.ks = parts >= 2 && tile_count(a, t) <= rten_hip_ctx::kSplitCounters ? parts : 0;
    return a.ks ? t : kNoTile;
}

} // namespace

int32_t rten_i8_dispatch_fast(rten_hip_ctx *ctx, void *args, double ops, double bytes) {
    FastArgs &a = *static_cast<FastArgs *>(args);
    // tile choice: the largest tile that still gives every CU a workgroup (the tile DMA of a workgroup tops out far below what the MFMAs could consume, so an
    // idle CU costs more than the extra operand re-reads of a smaller tile); tile order: consecutive workgroup ids (one XCD's share) walk the axis of the
    // SMALLER operand, so that the larger one is fetched into as few of the eight L2s as possible
    static const int env_tile = getenv("RTEN_I8_TILE") ? atoi(getenv("RTEN_I8_TILE")) : -1; // (tuning: 0 = 128x128, 1 = 128x64, 2 = 64x128, 3 = 64x64)
    const int setting = env_tile >= 0 ? env_tile : ctx->int8_tile >= 0 ? ctx->int8_tile : a.M <= 64 ? 2 : tile_count(a, T128x128) >= ctx->num_cus ? 0 : tile_count(a, T128x64) >= ctx->num_cus ? 1 : 3;
    const Tile tile = tile_of(setting, four_k_groups(ctx, a)); // (the plain kernels' choice)
    a.n_fastest = (double)a.a_bytes > (double)a.b_bytes ? 1 : 0;
    bool ok; // false: a quantized-output launch that was refused (the other forms always launch)
    if (a.q_out && a.in_stats) { // recompute form of a quantized output (QO == 2): the plain kernels' tile choice, nothing to fit
        ok = launch_tile<RECOMPUTE>(ctx, a, tile, ops, bytes);
    } else if (a.q_out) { // exchange form (QO == 1): the same tile choice, or the next larger one that fits the chip at once; else the caller runs the two-launch sequence
        const Tile larger = next_larger(tile);
        ok = launch_tile<EXCHANGE>(ctx, a, tile, ops, bytes) || (larger != kNoTile && launch_tile<EXCHANGE>(ctx, a, larger, ops, bytes));
    } else if (a.xf) { // quantize-on-load form (rten_hip_conv2d_int8_dql): one k-group on every tile
        ok = launch_tile<LOADQ>(ctx, a, tile_of(setting, false), ops, bytes);
    } else if (const Tile split = k_split_tile(ctx, a); split != kNoTile) {
        ok = launch_tile<KSPLIT>(ctx, a, split, ops, bytes);
    } else {
        ok = launch_tile<PLAIN>(ctx, a, tile, ops, bytes);
    }
    if (!ok) return RTEN_HIP_ERR_UNSUPPORTED;
    RTEN_LAUNCH_CHECK(ctx, "igemm_i8_fast_kernel launch");
    return RTEN_HIP_OK;
}

