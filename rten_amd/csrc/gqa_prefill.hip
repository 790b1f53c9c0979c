// Fused prefill for GroupQueryAttention: gqa_prefill_kernel<D>, D in {64, 128}, every call that would take the blocked-order composed path of gqa.hip (more
// than one query row, or one row with the gemv order off).  It runs after gqa_prepare_kernel, reads K and V from the present caches [B, KV, T, D] that launch
// wrote and Q in place (the rotated copy when rotary is on), and writes out[b, s, h] = softmax(mod(scale * Q K^T)) V for a strip of 64 query rows of one
// (batch, query head) in ONE launch.  No score leaves the compute unit: there is no score scratch.  seqlens_k and total are read on the device (lens()).
// The composed path (blocked GEMM, gqa_scores_kernel, blocked GEMM) order for order, hence its bits (tests/gqa_rules.py):
//   * score: one d-ascending v_mfma_f32_16x16x4_f32 chain from zero (one depth block), acc * scale;
//   * gqa_scores_kernel's modification with window() per row: the bias added inside [start, lim), every other column of [0, T) overwritten with -inf;
//   * softmax_row: max from f32::MIN by fmaxf, vm::exp_reduced(x - mx), sixteen partial sums (partial j: keys t % 16 == j, t ascending) folded
//     ((0 + a0) + a1) + ... + a15, inv = 1 / s, p = e * inv with NaN -> 0;
//   * PV: per depth block of 256 keys one t-ascending MFMA chain from zero, the first block stored, each later one added to the running total.
// Like the composed path it ranges over all T = P + S columns, so a right-padded item (kv_len < P + S) has the composed path's bits.
//
// Three sweeps, score tiles recomputed, and the lane mapping of attn_prefill_kernel (attention_prefill.hip, whose header derives it): 256 threads, wave w owns
// query rows 16 w .. 16 w + 15 of the strip, a key tile is 64 keys = 4 blocks j of 16, scores are computed transposed with a block's key rows permuted so that
// accumulator register r of lane (query = lane % 16, q = lane / 16) is key 16 j + 4 r + q of the tile: a fixed residue t % 16 == 4 r + q, so the ordered
// partials are in-lane adds, and the same register is the B operand of PV step 4 j + r.  Q stays in registers; one K tile (depth-permuted, XOR-swizzled rows)
// and one V tile ([key][D], swizzled by key % 4) in LDS, staged through one register buffer with 16-byte loads (4-byte loads when a cache is not 16-byte
// aligned); the depth-block total lives in `out`.  The G heads of a KV group are neighbouring workgroups (any G), then strips (last first), KV heads, batch.
//
// What is new here is the tile range each sweep walks.  window()'s start and lim do not fall with the row, so for a strip the tiles below
// lo = start(first row) / 64 and the tiles from hi = ceil(lim(last row) / 64) on hold -inf for EVERY row of the strip.
//   * Sweeps A and B walk [lo, hi) only.  A skipped tile would have offered -inf to fmaxf (nothing) and exp_reduced(-inf - mx) == +0 for every mx in
//     [f32::MIN, +inf] to partials that start at +0 and are never -0 (x + +0 == x for every x but -0): the argument of attention_prefill.hip's header.
//   * Sweep C.  On such a tile every probability is +0 whatever inv is (+0 * inv is +0, or NaN flushed to +0), so its PV steps are fma(+0, v, acc).  A chain
//     starts from +0, and an accumulator is never -0: +0 + (+-0) is +0, an exact cancellation rounds to +0, and only (-0) + (-0) gives -0.  With v finite the
//     product is +-0 and fma(+-0, finite, acc) leaves acc unchanged, bit for bit; so a wholly masked tile whose V rows are all finite changes nothing and
//     is skipped: no LDS staging, no score recomputation, no MFMA.  Whether they are finite is tested on the staging registers (exponent field all ones),
//     combined with one __syncthreads_or.  When a value is not finite only the score recomputation is skipped and the PV MFMAs run on zero probabilities, so
//     a NaN or Inf in a masked V row reaches the output as in the reference.  Tiles wholly at or beyond row past_len + S are zero rows that the prepare
//     launch of this same call wrote: skipped with no fetch.
//   * A depth block all of whose tiles were skipped is a block of +0: storing it first and adding the next to it gives the next block's bits (+0 + x == x, x
//     never -0), as does adding it later.  So the first depth block that is COMPUTED is the one stored and blocks that were not computed are not added.
//     [lo, hi) is never empty (lim > start for every row), so every row is stored.
// Rows past S in the last strip repeat the last row and are not stored.  No load leaves rows [0, T) of a cache head or columns [start, lim) of a bias row.
#include "gqa_common.h"
#include "vecmath.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int GP_ROWS = 64;   // query rows per workgroup
constexpr int GP_KEYS = 64;   // keys per tile
constexpr int GP_FOLD = 256;  // keys per PV depth block
constexpr int GP_THREADS = 256;
constexpr float NEG_INF = -__builtin_inff();

struct GqaPrefillArgs {
    GqaArgs a;
    int nstrips, vec_out, vec_kv; // vec_out: out takes 16-byte stores; vec_kv: both caches take 16-byte loads
};

template <int D>
__device__ __forceinline__ int k_at(int row, int pos) { return row * D + (pos ^ ((row & 15) << 2)); }

// rows [t0, t0 + 64) of a [T, D] matrix into registers; rows from T on are zero
template <int D>
__device__ __forceinline__ void fetch_tile(f32x4 (&reg)[D / 16], const float *base, int t0, int T, int tid, int vec) {
#pragma unroll
    for (int i = 0; i < D / 16; i++) {
        const int f = i * GP_THREADS + tid, row = f / (D / 4), dq = f % (D / 4);
        reg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t0 + row < T) {
            const float *src = base + (int64_t)(t0 + row) * D + dq * 4;
            if (vec) reg[i] = *reinterpret_cast<const f32x4 *>(src);
            else reg[i] = f32x4{src[0], src[1], src[2], src[3]};
        }
    }
}

template <int D>
__global__ __launch_bounds__(GP_THREADS, 2) void gqa_prefill_kernel(const GqaPrefillArgs pa) {
    constexpr int NR = D / 16; // Q registers (as f32x4), output blocks of 16 columns, 16-byte loads of a tile per thread
    __shared__ __attribute__((aligned(16))) float Ks[GP_KEYS * D];
    __shared__ __attribute__((aligned(16))) float Vs[GP_KEYS * D];
    const GqaArgs &p = pa.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, quad = lane >> 4;
    const int T = p.T;

    unsigned w = blockIdx.x;
    const int hg = (int)(w % (unsigned)p.G);
    w /= (unsigned)p.G;
    const int strip = pa.nstrips - 1 - (int)(w % (unsigned)pa.nstrips);
    w /= (unsigned)pa.nstrips;
    const int g = (int)(w % (unsigned)p.KV), b = (int)(w / (unsigned)p.KV);
    const int h = g * p.G + hg;
    const int s0 = strip * GP_ROWS;

    int kv_len, past_len;
    lens(p, b, kv_len, past_len);
    const int last = s0 + GP_ROWS - 1 < p.S ? s0 + GP_ROWS - 1 : p.S - 1;
    int kt_lo, kt_hi, unused;
    window(p, past_len, s0, kt_lo, unused);
    window(p, past_len, last, unused, kt_hi);
    kt_lo /= GP_KEYS;                                                // tiles below hold -inf for every row of the strip,
    kt_hi = (kt_hi + GP_KEYS - 1) / GP_KEYS;                         // and so do tiles from here on
    const int kt_end = (past_len + p.S + GP_KEYS - 1) / GP_KEYS;     // tiles from here on are zero rows of this call's prepare launch (kt_hi <= kt_end <= ceil(T / 64))
    const int s = s0 + wave * 16 + l15;
    const int srow = s < p.S ? s : p.S - 1; // rows past S repeat the last row and are not stored
    int start, lim;
    window(p, past_len, srow, start, lim);
    const float *brow = p.bias ? p.bias + b * p.bias_sb + h * p.bias_sh + srow * p.bias_sr : nullptr;
    const float *kb = p.pk + ((int64_t)b * p.KV + g) * T * D;
    const float *vb = p.pv + ((int64_t)b * p.KV + g) * T * D;

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
    float *const orow = p.out + (((int64_t)b * p.S + srow) * p.H + h) * D + 4 * quad;
    bool stored = false, dirty = false; // a depth block has been stored; this depth block has taken MFMAs (both uniform over the workgroup)

    for (int sweep = 0; sweep < 3; sweep++) { // A: maxima, B: partial sums, C: probabilities and PV
        const bool pv = sweep == 2;
        const int lo = pv ? 0 : kt_lo, hi = pv ? kt_end : kt_hi;
        f32x4 pre[NR]; // the tile in flight: K of the next tile in the band (in sweep C V of this one in between), V of the next tile outside it
        int ts = tid;
        asm volatile("" : "+v"(ts)); // (as for tl below)
        fetch_tile<D>(pre, lo >= kt_lo && lo < kt_hi ? kb : vb, lo * GP_KEYS, T, ts, pa.vec_kv);
        for (int kt = lo; kt < hi; kt++) {
            const int t0 = kt * GP_KEYS;
            const bool band = kt >= kt_lo && kt < kt_hi, more = kt + 1 < hi;
            const float *const next = kt + 1 >= kt_lo && kt + 1 < kt_hi ? kb : vb;
            // (an opaque copy: hoisted out of the tile loop, the staging addresses of every unrolled step take the registers the accumulators need)
            int tl = tid;
            asm volatile("" : "+v"(tl));
            f32x4 sc[4];
            bool run_pv = false;
            if (band) {
                __syncthreads(); // the previous tile is no longer read
#pragma unroll
                for (int i = 0; i < NR; i++) {
                    const int f = i * GP_THREADS + tl, row = f / (D / 4), dq = f % (D / 4), pos = 16 * (dq >> 2) + (dq & 3);
                    Ks[k_at<D>(row, pos)] = pre[i][0];
                    Ks[k_at<D>(row, pos + 4)] = pre[i][1];
                    Ks[k_at<D>(row, pos + 8)] = pre[i][2];
                    Ks[k_at<D>(row, pos + 12)] = pre[i][3];
                }
                __syncthreads();
                if (pv) fetch_tile<D>(pre, vb, t0, T, tl, pa.vec_kv);
                else if (more) fetch_tile<D>(pre, next, t0 + GP_KEYS, T, tl, pa.vec_kv);

                // S^T blocks j = 0..3 (16 keys x this wave's 16 queries), d ascending
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
                // sc[j][r] is key t0 + 16 j + 4 r + quad: the GEMM's store form, then the score modification (lim <= T: keys from T on are -inf)
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int t = t0 + 16 * j + 4 * r + quad;
                        float o = NEG_INF;
                        if (t >= start && t < lim) {
                            o = sc[j][r] * p.scale;
                            if (brow) o = o + brow[t];
                        }
                        sc[j][r] = o;
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
                    run_pv = true;
                }
            } else { // sweep C, a tile that is -inf for the whole strip: `pre` holds its V rows
                int wild = 0;
#pragma unroll
                for (int i = 0; i < NR; i++)
#pragma unroll
                    for (int c = 0; c < 4; c++) wild |= (__float_as_uint(pre[i][c]) & 0x7f800000u) == 0x7f800000u;
                // (also the barrier after which the previous tile's V is no longer read)
                if (__syncthreads_or(wild)) { // a NaN or Inf row: the PV steps run on the zero probabilities the scores would have given
#pragma unroll
                    for (int j = 0; j < 4; j++) sc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    run_pv = true;
                } else if (more) {
                    fetch_tile<D>(pre, next, t0 + GP_KEYS, T, tl, pa.vec_kv);
                }
            }
            if (run_pv) {
                // V of this tile (every wave is past the barriers above, hence done with the previous tile's V), then the next tile's K or V
#pragma unroll
                for (int i = 0; i < NR; i++) {
                    const int f = i * GP_THREADS + tl, row = f / (D / 4), dq = f % (D / 4);
                    *reinterpret_cast<f32x4 *>(Vs + row * D + ((dq * 4) ^ ((row & 3) << 4))) = pre[i];
                }
                __syncthreads();
                if (more) fetch_tile<D>(pre, next, t0 + GP_KEYS, T, tl, pa.vec_kv);
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
                dirty = true;
            }
            if (dirty && ((kt + 1) % (GP_FOLD / GP_KEYS) == 0 || !more)) { // a computed depth block ends: the first is stored, the rest are added
#pragma unroll
                for (int jn = 0; jn < NR; jn++) {
                    if (s < p.S) {
                        if (pa.vec_out) {
                            f32x4 *o4 = reinterpret_cast<f32x4 *>(orow + 16 * jn);
                            *o4 = stored ? *o4 + oc[jn] : oc[jn];
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; r++) orow[16 * jn + r] = stored ? orow[16 * jn + r] + oc[jn][r] : oc[jn][r];
                        }
                    }
                    oc[jn] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                stored = true;
                dirty = false;
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

bool rten_gqa_prefill_covers(const GqaArgs &a) {
    return (a.D == 64 || a.D == 128) && ceil_div64(a.S, GP_ROWS) * a.B * a.H <= 0x7fffffff;
}

int32_t rten_gqa_prefill_launch(rten_hip_ctx *ctx, const GqaArgs &a) {
    GqaPrefillArgs pa = {};
    pa.a = a;
    pa.nstrips = (int)ceil_div64(a.S, GP_ROWS);
    pa.vec_out = ((uintptr_t)a.out & 15u) == 0;
    pa.vec_kv = (((uintptr_t)a.pk | (uintptr_t)a.pv) & 15u) == 0;
    const double rows = (double)a.B * a.H * a.S, kv = 8.0 * a.B * a.KV * (double)a.T * a.D;
    ProfScope ps(ctx, "gqa_prefill_kernel", 4.0 * rows * a.T * a.D, kv + 8.0 * rows * a.D);
    const dim3 grid((unsigned)((int64_t)a.B * a.H * pa.nstrips)), block(GP_THREADS);
    if (a.D == 64) hipLaunchKernelGGL(gqa_prefill_kernel<64>, grid, block, 0, ctx->stream, pa);
    else hipLaunchKernelGGL(gqa_prefill_kernel<128>, grid, block, 0, ctx->stream, pa);
    RTEN_LAUNCH_CHECK(ctx, "gqa_prefill_kernel");
    return RTEN_HIP_OK;
}
