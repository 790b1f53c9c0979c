// Fused prefill for Attention (ai.onnx, opset 23): attn_prefill_kernel<D>, D == Dv in {64, 128}, more than one query row (or one row in the blocked order).
// out[b, h, s] = softmax(mod(scale * Q K^T)) V for a strip of 64 query rows of one (batch, query head) in ONE launch; no score leaves the compute unit.
// The composed path of attention_kv.hip (blocked GEMM, attn_scores_kernel, blocked GEMM) order for order, hence its bits (tests/attention_rules.py):
//   * score: one d-ascending v_mfma_f32_16x16x4_f32 chain from zero (D <= 256: one depth block), acc * scale, modified() with masked_from();
//   * softmax_row: max from f32::MIN by fmaxf, vm::exp_reduced(x - mx), sixteen partial sums (partial j: keys t % 16 == j, t ascending) folded
//     ((0 + a0) + a1) + ... + a15, inv = 1 / s, p = e * inv with NaN -> 0;
//   * PV: per depth block of 256 keys one t-ascending MFMA chain from zero, the first block stored, each later one added to the running total.
//     Every key of [0, T) takes part (a masked key with probability +0: a NaN in its V row propagates).
//
// Three sweeps.  The row softmax is three passes over a whole row, not an online one, and 64 rows x T scores do not fit LDS, so the score tiles are
// RECOMPUTED, not stored: sweep A takes the row maxima, sweep B forms e and the sixteen ordered partials and then inv, sweep C forms p and feeds the PV
// MFMAs.  The same instruction sequence on the same operands gives the same score bits each time.
//
// Mapping (the one of sdpa_fused16_kernel, attention_fused.hip, walked over key tiles).  256 threads, wave w owns query rows 16 w .. 16 w + 15 of the
// strip; a key tile is 64 keys = 4 blocks j of 16.  Scores are computed transposed, S^T = K Q^T, with a block's key rows permuted: MFMA row 4 q + r
// carries key 16 j + 4 r + q, so accumulator register r of lane (query = lane % 16, q = lane / 16) is key 16 j + 4 r + q of the tile.  Key tiles start
// at multiples of 64, so that register sits on the fixed residue t % 16 == 4 r + q: the ordered partials are in-lane adds over ascending blocks and
// tiles, and the fold walks the four quads once per row at the end of sweep B.  The same register is the B operand (k index q) of PV step 4 j + r of
// out^T = V^T P^T: probabilities never move between lanes.  The maxima are reduced across the four quads once, at the end of sweep A.
// Q: the wave's 16 rows stay in registers for the whole kernel (depth d = 4 step + q in lane quad q: D / 4 registers).
// LDS: one K tile (rows of D floats, depth d = 16 a + 4 i + g stored at 16 a + 4 g + i, 16-byte groups XOR-swizzled by the row: one ds_read_b128 = the
// operands of four MFMA steps) and one V tile ([key][D], 16-float groups XOR-swizzled by key % 4); 16-byte global loads, the next tile fetched into
// registers while this one is computed.  512 D bytes: 64 KiB at D = 128, two workgroups per compute unit.
//
// Skipping.  A key tile at or beyond masked_from() of EVERY row of the strip holds -inf only: nothing for fmaxf, and exp_reduced(-inf - mx) is +0 for
// every mx in [f32::MIN, +inf] (x - mx is -inf there, below the cut-off that selects 0.f; vecmath.h), added to partials that are never -0.  Sweeps A and
// B stop at the strip's last unmasked tile (causal: about half of the tiles of a first prompt).  Sweep C skips nothing.  nonpad_kv_seqlen is read on
// the device with the clamp of nonpad_of(); nothing is read back.
// Workgroup order: the G heads of a KV group are neighbours, then the strips (longest causal strip first), then KV heads, then batch items: a K / V
// tile fetched for one workgroup is an L2 hit for the others.
#include "attention_common.h"
#include "vecmath.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int PF_ROWS = 64;   // query rows per workgroup
constexpr int PF_KEYS = 64;   // keys per tile
constexpr int PF_FOLD = 256;  // keys per PV depth block
constexpr int PF_THREADS = 256;

struct PrefillArgs {
    AttnArgs a;
    const float *kc, *vc; // K and V as contiguous [B, Hkv, T, D]
    int nstrips, vec_out; // vec_out: out takes 16-byte stores
};

template <int D>
__device__ __forceinline__ int k_at(int row, int pos) { return row * D + (pos ^ ((row & 15) << 2)); }

// rows [t0, t0 + 64) of a [T, D] matrix into registers, 16 bytes per load; rows from T on are zero
template <int D>
__device__ __forceinline__ void fetch_tile(f32x4 (&reg)[D / 16], const float *base, int t0, int T, int tid) {
#pragma unroll
    for (int i = 0; i < D / 16; i++) {
        const int f = i * PF_THREADS + tid, row = f / (D / 4), dq = f % (D / 4);
        reg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t0 + row < T) reg[i] = *reinterpret_cast<const f32x4 *>(base + (int64_t)(t0 + row) * D + dq * 4);
    }
}

template <int D>
__global__ __launch_bounds__(PF_THREADS, 2) void attn_prefill_kernel(const PrefillArgs pa) {
    constexpr int NR = D / 16; // Q registers (as f32x4), output blocks of 16 columns, 16-byte loads of a tile per thread
    __shared__ __attribute__((aligned(16))) float Ks[PF_KEYS * D];
    __shared__ __attribute__((aligned(16))) float Vs[PF_KEYS * D];
    const AttnArgs &p = pa.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, quad = lane >> 4;
    const int T = p.T;

    unsigned w = blockIdx.x;
    const int hg = (int)(w % (unsigned)p.G);
    w /= (unsigned)p.G;
    const int strip = pa.nstrips - 1 - (int)(w % (unsigned)pa.nstrips);
    w /= (unsigned)pa.nstrips;
    const int g = (int)(w % (unsigned)p.Hkv), b = (int)(w / (unsigned)p.Hkv);
    const int h = g * p.G + hg;
    const int s0 = strip * PF_ROWS;

    const int np = nonpad_of(p, b);
    const int last = s0 + PF_ROWS - 1 < p.Sq ? s0 + PF_ROWS - 1 : p.Sq - 1;
    const int nt = (T + PF_KEYS - 1) / PF_KEYS;
    const int nt_ab = (masked_from(p, np, last) + PF_KEYS - 1) / PF_KEYS; // masked_from() does not fall with the row: tiles from here on are -inf for the whole strip
    const int s = s0 + wave * 16 + l15;
    const int srow = s < p.Sq ? s : p.Sq - 1; // rows past Sq repeat the last row and are not stored
    const int from = masked_from(p, np, srow);
    const void *mrow = p.mask_kind != RTEN_HIP_ATTN_MASK_NONE ? mask_row(p, b, h, srow) : nullptr;
    const float *kb = pa.kc + ((int64_t)b * p.Hkv + g) * T * D;
    const float *vb = pa.vc + ((int64_t)b * p.Hkv + g) * T * D;

    // Q: register i of group a4 is depth 16 a4 + 4 i + quad = MFMA step 4 a4 + i, k index quad
    f32x4 qf[NR];
    {
        const float *qr = p.q + b * p.q_sb + h * p.q_sh + srow * p.q_ss + quad;
#pragma unroll
        for (int a4 = 0; a4 < NR; a4++)
#pragma unroll
            for (int i = 0; i < 4; i++) qf[a4][i] = qr[16 * a4 + 4 * i];
    }
    const int krow = 4 * (l15 & 3) + (l15 >> 2); // MFMA row l15 = 4 q' + r' of block j carries key 16 j + 4 r' + q'

    float mx = -3.40282347e+38f; // f32::MIN (softmax.rs:181)
    float part[4] = {0.f, 0.f, 0.f, 0.f}; // partial 4 r + quad of the 16-lane order
    float inv = 0.f;
    f32x4 oc[NR];
#pragma unroll
    for (int jn = 0; jn < NR; jn++) oc[jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    // register r of block jn is column 16 jn + 4 quad + r of query row s.  The running total of the depth blocks lives in `out` itself: every lane
    // re-reads only what it stored
    float *const orow = p.out + b * p.o_sb + h * p.o_sh + srow * p.o_ss + 4 * quad;

    for (int sweep = 0; sweep < 3; sweep++) { // A: maxima, B: partial sums, C: probabilities and PV
        const bool pv = sweep == 2;
        const int tiles = pv ? nt : nt_ab;
        f32x4 pre[NR]; // the tile in flight: K of the next tile, in sweep C V of this one in between
        int ts = tid;
        asm volatile("" : "+v"(ts)); // (as for tl below)
        if (tiles > 0) fetch_tile<D>(pre, kb, 0, T, ts);
        for (int kt = 0; kt < tiles; kt++) {
            const int t0 = kt * PF_KEYS;
            // (opaque copies: hoisted out of the tile loop, the staging and mask addresses of every unrolled step take ~170 registers and spill)
            int tl = tid;
            int64_t m_st = p.m_st;
            asm volatile("" : "+v"(tl), "+s"(m_st));
            __syncthreads(); // the previous tile is no longer read
#pragma unroll
            for (int i = 0; i < NR; i++) {
                const int f = i * PF_THREADS + tl, row = f / (D / 4), dq = f % (D / 4), pos = 16 * (dq >> 2) + (dq & 3);
                Ks[k_at<D>(row, pos)] = pre[i][0];
                Ks[k_at<D>(row, pos + 4)] = pre[i][1];
                Ks[k_at<D>(row, pos + 8)] = pre[i][2];
                Ks[k_at<D>(row, pos + 12)] = pre[i][3];
            }
            __syncthreads();
            if (pv) fetch_tile<D>(pre, vb, t0, T, tl);
            else if (kt + 1 < tiles) fetch_tile<D>(pre, kb, t0 + PF_KEYS, T, tl);

            // S^T blocks j = 0..3 (16 keys x this wave's 16 queries), d ascending
            f32x4 sc[4];
#pragma unroll
            for (int j = 0; j < 4; j++) sc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int a4 = 0; a4 < NR; a4++) {
                f32x4 kf[4];
#pragma unroll
                for (int j = 0; j < 4; j++) kf[j] = *reinterpret_cast<const f32x4 *>(Ks + k_at<D>(16 * j + krow, 16 * a4 + 4 * quad));
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) sc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j][i], qf[a4][i], sc[j], 0, 0, 0);
            }
            // sc[j][r] is key t0 + 16 j + 4 r + quad: the GEMM's store form, then the score modification; keys from T on are -inf (e and p +0)
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int t = t0 + 16 * j + 4 * r + quad;
                    const float o = sc[j][r] * p.scale;
                    sc[j][r] = t < T ? modified_at(p, o, mrow, t * m_st, t, from) : NEG_INF;
                }
            if (sweep == 0) {
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int r = 0; r < 4; r++) mx = fmaxf(mx, sc[j][r]);
            } else if (sweep == 1) {
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int r = 0; r < 4; r++) part[r] = part[r] + vm::exp_reduced(sc[j][r] - mx);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        float pr = vm::exp_reduced(sc[j][r] - mx) * inv;
                        if (!(pr == pr)) pr = 0.f; // flush_nans_to_zero (attention.rs:551)
                        sc[j][r] = pr;
                    }
                // V of this tile (every wave is past the barriers above, hence done with the previous tile's V), then K of the next tile
#pragma unroll
                for (int i = 0; i < NR; i++) {
                    const int f = i * PF_THREADS + tl, row = f / (D / 4), dq = f % (D / 4);
                    *reinterpret_cast<f32x4 *>(Vs + row * D + ((dq * 4) ^ ((row & 3) << 4))) = pre[i];
                }
                __syncthreads();
                if (kt + 1 < tiles) fetch_tile<D>(pre, kb, t0 + PF_KEYS, T, tl);
                // out^T[dv][s] += V^T[dv][key] P^T[key][s]: step 4 j + r takes keys 4 (4 j + r) + {0..3} of the tile, ascending
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float *vr = Vs + (16 * j + 4 * r + quad) * D; // (key % 4 == quad: the swizzle term is per lane)
#pragma unroll
                        for (int jn = 0; jn < NR; jn++)
                            oc[jn] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[(16 * jn + l15) ^ (quad << 4)], sc[j][r], oc[jn], 0, 0, 0);
                    }
                if ((kt + 1) % (PF_FOLD / PF_KEYS) == 0 || kt + 1 == tiles) { // a depth block ends: the first is stored, the rest are added
                    const bool first = kt < PF_FOLD / PF_KEYS;
#pragma unroll
                    for (int jn = 0; jn < NR; jn++) {
                        if (s < p.Sq) {
                            if (pa.vec_out) {
                                f32x4 *o4 = reinterpret_cast<f32x4 *>(orow + 16 * jn);
                                *o4 = first ? oc[jn] : *o4 + oc[jn];
                            } else {
#pragma unroll
                                for (int r = 0; r < 4; r++) orow[16 * jn + r] = first ? oc[jn][r] : orow[16 * jn + r] + oc[jn][r];
                            }
                        }
                        oc[jn] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
            }
        }
        if (sweep == 0) {
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        } else if (sweep == 1) { // fold partials 0..15 left to right; partial 4 r + q lives in quad q
            float pq[4][4];
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int r = 0; r < 4; r++) pq[q][r] = __shfl(part[r], 16 * q + l15, 64);
            float ssum = 0.f;
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int q = 0; q < 4; q++) ssum = ssum + pq[q][r];
            inv = 1.0f / ssum;
        }
    }
}

} // namespace

bool rten_attn_prefill_covers(const AttnArgs &a) {
    return a.D == a.Dv && (a.D == 64 || a.D == 128) && ceil_div64(a.Sq, PF_ROWS) * a.B * a.Hq <= 0x7fffffff;
}

int32_t rten_attn_prefill_launch(rten_hip_ctx *ctx, const AttnArgs &a, const float *kc, const float *vc) {
    PrefillArgs pa = {};
    pa.a = a;
    pa.kc = kc;
    pa.vc = vc;
    pa.nstrips = (int)ceil_div64(a.Sq, PF_ROWS);
    pa.vec_out = ((uintptr_t)a.out & 15u) == 0 && a.o_sb % 4 == 0 && a.o_sh % 4 == 0 && a.o_ss % 4 == 0;
    const double rows = (double)a.B * a.Hq * a.Sq, kv = 8.0 * a.B * a.Hkv * (double)a.T * a.D;
    ProfScope ps(ctx, "attn_prefill_kernel", 4.0 * rows * a.T * a.D, kv + 8.0 * rows * a.D);
    const dim3 grid((unsigned)((int64_t)a.B * a.Hq * pa.nstrips)), block(PF_THREADS);
    if (a.D == 64) hipLaunchKernelGGL(attn_prefill_kernel<64>, grid, block, 0, ctx->stream, pa);
    else hipLaunchKernelGGL(attn_prefill_kernel<128>, grid, block, 0, ctx->stream, pa);
    RTEN_LAUNCH_CHECK(ctx, "attn_prefill_kernel");
    return RTEN_HIP_OK;
}
