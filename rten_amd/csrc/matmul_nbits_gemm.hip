// MatMulNBits for M = batch * rows >= 2: the 4-bit weights are dequantised on the way into LDS and multiplied by v_mfma_f32_16x16x4_f32 chains -- no f32 copy
// of the weights in memory, no scratch, nothing allocated (legal inside a capture).  The reference dequantises while it packs the B panel
// (rten-gemm/src/packing.rs:229-318, src/ops/matmul/contrib.rs:84-99); this is that, with LDS as the panel.
//
// Arithmetic (rten-gemm/src/lib.rs:1008-1013, kernels/simd_generic.rs:326-367, packing.rs:300-312): a weight is (float)(q - 8) * scale, one rounded multiply; an output element is a k-ordered
// FMA chain from +0.0 over each 256-deep block (a chain of v_mfma_f32_16x16x4_f32 is one: tools/probes/mfma_16x16x4_order.hip); the first block's sum is
// stored as it is, every later one added with a separate rounded add in block order.  K is a multiple of 16 (block size >= 16 divides it) and no MFMA is
// issued for depths at or beyond K: a padded fma(0, 0, acc) would turn a -0.0 accumulator into +0.0.  Rows >= M and columns >= N of a tile are computed on
// the clamped (last) row / column and never stored: rows and columns are independent chains.
//
// Work split <MT, NT, KW>, 256 threads = 4 waves, NT * KW = 4: a workgroup owns a 16 MT x 16 NT tile of C over the whole K.  Wave w owns column block
// w / KW (all MT row blocks: MT interleaved chains) and the depth blocks congruent to w % KW: the KW waves of a column block run KW depth blocks at once, so
// a 16-row product puts ceil(N / 16) workgroups of four busy waves on the chip instead of ceil(N / 64).  Block sums meet in LDS: at the end of a round of KW
// depth blocks every wave parks its sums, and the wave with w % KW == 0 adds them to its running total in block order.
//
// Data path.  A stage is 64 depths of each of the KW depth blocks in flight ("slabs"): 16 NT columns x 64 KW depths = 4096 weights, 16 per thread.  A thread
// fetches 8 bytes = 16 consecutive depths of one column (inside one quantisation block, since 16 divides the block size) and that block's scale, splits the
// nibbles with two masks and v_cvt_f32_ubyteN, subtracts 8, multiplies once and writes four ds_write_b128.  The A tile (16 MT rows x 64 KW depths) goes the
// same way: 16 consecutive depths of a row per unit, four 16-byte global loads where the base is 16-byte aligned, four ds_write_b128.
// LDS image of an operand row per slab: 64 depths = 16 slots of 4 floats; depth 16 j + 4 i + g sits at float i of slot 4 j + g, and slots are XOR-swizzled by the
// row (slot ^ (row & 15)): lane (row = lane % 16, g = lane / 16) reads the operands of MFMAs 4 j .. 4 j + 3 with ONE conflict-free ds_read_b128, and the loaders'
// 16-byte writes are conflict free too.  Two buffers: the next stage's global loads are issued before the current stage's MFMA chain and dequantised into
// the other buffer behind it; one barrier per stage.
#include "internal.h"

#include <cstdlib>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct NbitsArgs {
    const float *a;
    const uint8_t *q;
    const float *sc;
    float *y;
    int M, N, K, lbs; // lbs = log2(block size)
    int a_vec, q_vec; // A 16-byte aligned / quant 8-byte aligned: vector loads
};

// float index of (slab, operand row, slot) in an image of ROWS rows per slab
template <int ROWS>
__device__ __forceinline__ int img_at(int slab, int row, int slot) { return ((slab * ROWS + row) * 16 + (slot ^ (row & 15))) * 4; }

template <int MT, int NT, int KW>
__global__ __launch_bounds__(256) void nbits_gemm_kernel(const NbitsArgs p) {
    static_assert(NT * KW == 4 && (MT * KW) % 4 == 0, "four waves; whole A units per thread");
    constexpr int RA = 16 * MT, RB = 16 * NT; // operand rows per slab
    constexpr int UA = MT * KW / 4;           // A units (16 depths of a row) per thread and stage
    constexpr int A_IMG = KW * RA * 64, B_IMG = KW * RB * 64, STAGE = A_IMG + B_IMG;
    constexpr int PARK = KW > 1 ? 4 * MT * 256 : 4; // parked block sums: [wave][row block][lane] x 4 floats
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE + PARK];
    float *park = smem + 2 * STAGE;

    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, quad = lane >> 4;
    const int kw = wave % KW, cb = wave / KW;
    const int n0 = blockIdx.x * RB, m0 = blockIdx.y * RA;
    const int K = p.K;
    const int nblk = (K + 255) >> 8, rounds = (nblk + KW - 1) / KW, nst = rounds * 4;

    // loader roles.  B: thread = (slab, column, 16-depth group); A: UA units of (slab, row, 16-depth group).  Columns / rows past the edge are clamped.
    const int jb = t & 3, bcol = (t >> 2) % RB, bslab = t / (4 * RB);
    const int gcol = n0 + bcol < p.N ? n0 + bcol : p.N - 1;
    const uint8_t *qcol = p.q + (long long)gcol * (K >> 1);
    const float *scol = p.sc + (long long)gcol * (K >> p.lbs);
    int ja[UA], rowa[UA], slaba[UA];
    const float *arow[UA];
#pragma unroll
    for (int u = 0; u < UA; u++) {
        const int f = u * 256 + t;
        ja[u] = f & 3; rowa[u] = (f >> 2) % RA; slaba[u] = f / (4 * RA);
        const int gr = m0 + rowa[u] < p.M ? m0 + rowa[u] : p.M - 1;
        arow[u] = p.a + (long long)gr * K;
    }

    unsigned qlo = 0, qhi = 0;
    float scale = 0.f;
    f32x4 av[UA][4];
    // first depth of (stage it, slab)
    auto depth0 = [&](int it, int slab) { return ((((it >> 2) * KW) + slab) << 8) + 64 * (it & 3); };

    auto fetch = [&](int it) {
        const int k = depth0(it, bslab) + 16 * jb;
        if (k < K) {
            const uint8_t *qp = qcol + (k >> 1);
            if (p.q_vec) {
                const uint2 w = *reinterpret_cast<const uint2 *>(qp);
                qlo = w.x; qhi = w.y;
            } else {
                qlo = qp[0] | (qp[1] << 8) | (qp[2] << 16) | ((unsigned)qp[3] << 24);
                qhi = qp[4] | (qp[5] << 8) | (qp[6] << 16) | ((unsigned)qp[7] << 24);
            }
            scale = scol[k >> p.lbs];
        }
#pragma unroll
        for (int u = 0; u < UA; u++) {
            const int ka = depth0(it, slaba[u]) + 16 * ja[u];
            if (ka < K) {
                const float *ap = arow[u] + ka;
                if (p.a_vec) {
#pragma unroll
                    for (int i = 0; i < 4; i++) av[u][i] = *reinterpret_cast<const f32x4 *>(ap + 4 * i);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) av[u][i] = (f32x4){ap[4 * i], ap[4 * i + 1], ap[4 * i + 2], ap[4 * i + 3]};
                }
            }
        }
    };

    // dequantise / transpose what fetch(it) brought and write it into buffer it & 1
    auto stash = [&](int it) {
        float *Ab = smem + (it & 1) * STAGE, *Bb = Ab + A_IMG;
        if (depth0(it, bslab) + 16 * jb < K) {
            // depth d = 4 i + g of the group is nibble d & 1 of byte d >> 1: slot g holds depths g, 4 + g, 8 + g, 12 + g = bytes (g >> 1) + {0, 2, 4, 6}
            const unsigned l0 = qlo & 0x0F0F0F0Fu, h0 = (qlo >> 4) & 0x0F0F0F0Fu, l1 = qhi & 0x0F0F0F0Fu, h1 = (qhi >> 4) & 0x0F0F0F0Fu;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const unsigned w0 = (g & 1) ? h0 : l0, w1 = (g & 1) ? h1 : l1;
                const int sh = 8 * (g >> 1);
                f32x4 w;
                w[0] = ((float)((w0 >> sh) & 0xFFu) - 8.0f) * scale;
                w[1] = ((float)((w0 >> (sh + 16)) & 0xFFu) - 8.0f) * scale;
                w[2] = ((float)((w1 >> sh) & 0xFFu) - 8.0f) * scale;
                w[3] = ((float)((w1 >> (sh + 16)) & 0xFFu) - 8.0f) * scale;
                *reinterpret_cast<f32x4 *>(Bb + img_at<RB>(bslab, bcol, 4 * jb + g)) = w;
            }
        }
#pragma unroll
        for (int u = 0; u < UA; u++) {
            if (depth0(it, slaba[u]) + 16 * ja[u] < K) {
#pragma unroll
                for (int g = 0; g < 4; g++)
                    *reinterpret_cast<f32x4 *>(Ab + img_at<RA>(slaba[u], rowa[u], 4 * ja[u] + g)) = (f32x4){av[u][0][g], av[u][1][g], av[u][2][g], av[u][3][g]};
            }
        }
    };

    f32x4 acc[MT], tot[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) { acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; tot[m] = acc[m]; }

    // this wave's slab of stage `it`: 16 MFMAs per row block, none at or beyond K (the test is uniform over the wave)
    auto compute = [&](int it) {
        const float *Ab = smem + (it & 1) * STAGE, *Bb = Ab + A_IMG;
        const int k0 = depth0(it, kw);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (k0 + 16 * j < K) {
                const f32x4 b = *reinterpret_cast<const f32x4 *>(Bb + img_at<RB>(kw, cb * 16 + l15, 4 * j + quad));
                f32x4 a[MT];
#pragma unroll
                for (int m = 0; m < MT; m++) a[m] = *reinterpret_cast<const f32x4 *>(Ab + img_at<RA>(kw, m * 16 + l15, 4 * j + quad));
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int m = 0; m < MT; m++) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][i], b[i], acc[m], 0, 0, 0);
            }
        }
    };

    // end of round r: the finished block sums leave the accumulators (KW == 1: straight into the total)
    auto block_end = [&](int r) {
#pragma unroll
        for (int m = 0; m < MT; m++) {
            if constexpr (KW == 1) {
                if (r == 0) tot[m] = acc[m];
                else tot[m] = tot[m] + acc[m];
            } else {
                *reinterpret_cast<f32x4 *>(park + ((wave * MT + m) * 64 + lane) * 4) = acc[m];
            }
            acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    // behind the barrier that follows block_end(r): the first wave of a column block adds the round's sums in block order
    auto fold_in = [&](int r) {
        if constexpr (KW > 1) {
            if (kw != 0) return;
#pragma unroll
            for (int s = 0; s < KW; s++) {
                const int blk = r * KW + s;
                if (blk < nblk) {
#pragma unroll
                    for (int m = 0; m < MT; m++) {
                        const f32x4 v = *reinterpret_cast<const f32x4 *>(park + (((cb * KW + s) * MT + m) * 64 + lane) * 4);
                        if (blk == 0) tot[m] = v;
                        else tot[m] = tot[m] + v;
                    }
                }
            }
        }
    };

    fetch(0);
    stash(0);
    __syncthreads();
    for (int it = 0; it < nst; it++) {
        if (it && !(it & 3)) fold_in((it >> 2) - 1);
        if (it + 1 < nst) fetch(it + 1);
        compute(it);
        if ((it & 3) == 3) block_end(it >> 2);
        if (it + 1 < nst) stash(it + 1);
        __syncthreads();
    }
    fold_in(rounds - 1);

    // accumulator element r of row block m: row 16 m + 4 quad + r, column l15 of the wave's column block
    if (kw != 0) return;
    const int col = n0 + cb * 16 + l15;
    if (col >= p.N) return;
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = m0 + m * 16 + 4 * quad + r;
            if (row < p.M) p.y[(long long)row * p.N + col] = tot[m][r];
        }
}

template <int MT, int NT, int KW>
void launch(rten_hip_ctx *ctx, const NbitsArgs &a) {
    const dim3 grid((unsigned)((a.N + 16 * NT - 1) / (16 * NT)), (unsigned)((a.M + 16 * MT - 1) / (16 * MT)));
    hipLaunchKernelGGL((nbits_gemm_kernel<MT, NT, KW>), grid, dim3(256), 0, ctx->stream, a);
}

} // namespace

// The calls the kernel takes: block sizes up to 256 (16 divides every one) and no more 16-row tiles than a grid's second dimension holds.
bool rten_nbits_gemm_covers(long long m, int block_size) { return m >= 2 && m <= 16 * 65535LL && block_size <= 256; }

// The automatic rule: the fused kernel up to NBITS_FUSED_MAX_M rows, the last measured row count at which it beat expand + GEMM on all three matrices of
// docs/KERNELS.md 4.20; at 384, 512 and 2048 rows each route wins on some of them.  A matrix of fewer than 16 columns does not fill one MFMA column block
// and was not measured: it keeps the older route (which tests/test_gpu_range.py holds to the numeric envelope at 8 columns).
constexpr long long NBITS_FUSED_MAX_M = 256;
bool rten_nbits_gemm_pays(long long m, int n) { return m <= NBITS_FUSED_MAX_M && n >= 16; }

// The tile, by the measured cost of a 4096-deep workgroup (docs/KERNELS.md 4.20): a 16 x 16 grid costs 0.0416 us per workgroup, a 64 x 64 grid 106 us for anything up
// to one workgroup per compute unit -- so 16 x 16 tiles, whose four waves run four depth blocks at once, while their grid stays below 10 workgroups per compute
// unit (the cheaper tile at every shape of profiles/r22/matmul_nbits_forced_tile{16,64}.json), and always up to 32 rows, where a 64-row tile is at least half
// padding.  RTEN_HIP_NBITS_TILE = 1 / 4 forces the 16 x 16 / 64 x 64 tile (tuning, and the tests
// of the larger tile at small shapes).  The caller has checked rten_nbits_gemm_covers.
int32_t rten_launch_nbits_gemm(rten_hip_ctx *ctx, long long m, int k, int n, int block_size, const float *a, const uint8_t *q, const float *sc, float *y) {
    const char *env = getenv("RTEN_HIP_NBITS_TILE");
    const int forced = env ? atoi(env) : 0;
    const long long w16 = ((m + 15) / 16) * ((n + 15) / 16);
    const int mt = forced == 1 || forced == 4 ? forced : (m <= 32 || w16 < 10LL * ctx->num_cus) ? 1 : 4, nt = mt;
    NbitsArgs p = {a, q, sc, y, (int)m, n, k, __builtin_ctz((unsigned)block_size), ((uintptr_t)a & 15u) == 0, ((uintptr_t)q & 7u) == 0};
    const double col_tiles = (double)((n + 16 * nt - 1) / (16 * nt));
    char kname[48];
    snprintf(kname, sizeof kname, "nbits_gemm_kernel<%d,%d,%d>", mt, nt, 4 / nt);
    ProfScope ps(ctx, kname, 2.0 * (double)m * k * (double)n,
                 (double)n * k / 2 + 4.0 * ((double)n * (k / block_size) + col_tiles * (double)m * k + (double)m * n));
    if (mt == 1) launch<1, 1, 4>(ctx, p);
    else launch<4, 4, 1>(ctx, p);
    RTEN_LAUNCH_CHECK(ctx, "nbits_gemm_kernel launch");
    return RTEN_HIP_OK;
}
