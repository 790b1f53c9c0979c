// NonMaxSuppression (src/ops/non_max_suppression.rs:40-188): the reference's rule, which is NOT textbook per-class NMS.
//
//   candidates, in (n, b) order: class = arg-max over scores[n, :, b] under f32::total_cmp, the LAST maximal class; dropped when max_score < score_threshold
//   (IEEE: a NaN score stays); corners [t, l, b, r], from [cx, cy, w, h] as [cy - h/2, cx - w/2, cy + h/2, cx + w/2], one rounding per operation.
//   iou(p, q) = area(intersection) / area(HULL) with area = max(b - t, 0) * max(r - l, 0), min / max ignoring a NaN operand; 0 / 0 = NaN compares false.
//   ONE `selected` list for every image and class.  A candidate p walks it in order; at a member q with iou >= iou_threshold: score_p > score_q removes q and
//   the walk goes on, anything else rejects p and stops the walk -- what was removed before stays removed.  A candidate never rejected is appended.
//   The list is then stably sorted by score descending (total order) and, with a cap, the first `max` rows of each class are kept (counted across images).
//
// Removal keeps the list's order and a new member goes to its end, so the list is always the alive candidates in candidate order: it is a bit per candidate.
// Four steps, every launch on the context's stream:
//   1. nms_class_kernel, a thread per (n, b), consecutive threads on consecutive b (the walk over scores[n, c, :] is coalesced): class, score, the score
//      test, and the number of candidates of the workgroup.  nms_offsets_kernel (one workgroup) scans those counts; nms_gather_kernel recomputes each
//      thread's rank inside its workgroup and writes the candidate -- corners, score, class, n * B + b -- at its place.  Order is (n, b); no atomics.
//   2. nms_resolve_kernel, ONE workgroup of 16 waves: the loop above is serial by contract (whether p joins depends on every decision before it).  Word w of
//      `alive` belongs to wave w % 16 and there to one lane, always: only that thread ever reads or writes the word, so `alive` needs no cross-thread ordering.
//      For candidate p a wave loads 64 of its words at once (a lane per word) and then takes the words that HAVE a member one at a time, a lane per member: the
//      iou of p against the alive q < p only -- the pair masks of the textbook bit-matrix form, restricted to the members that exist, a few hundred of 8400
//      candidates in a detector -- with the word's removable members (iou >= thr and score_p > score_q) and its first blocker (iou >= thr otherwise) from two
//      ballots -- or, where the fullest of the 64 words has fewer members than there are words with any (a sparse list), every lane walks its own word.
//      A wave stops at its first blocker.  j = the workgroup's smallest blocker (one LDS slot per wave, ONE barrier per candidate: the slots
//      alternate).  No j: alive &= ~removable, alive[p] = 1.  Else alive &= ~(removable & below(j)).  The survivors are then written in order as 64-bit keys
//      (~total-order key of the score << 32 | candidate index).
//   3. nms_order_kernel, ONE workgroup: a bitonic sort of the keys (unique, so the order is the stable order: score descending, then (n, b)), then the
//      per-class cap -- a running count per class, a chunk of NMS_ORDER_THREADS sorted rows at a time -- and the rows [n, class, b], compacted in order.
//   4. the row count comes back through a host pointer: one 4-byte copy and the only synchronisation.  Rows past the count are never written.
// Scratch (the context's auxiliary buffer) depends on N * B and C only, so nothing is read back between the steps.
// The price of not materialising the pair masks: where little is suppressed (nearly every candidate alive) all of the M^2 / 2 pair evaluations run inside
// the one-workgroup loop, on one compute unit -- seconds for a few hundred thousand candidates, as ONE long-running kernel.  A bit-matrix form, whose masks
// are built over the whole chip, bounds that case and is the form to build if such inputs matter; a detector's score threshold leaves hundreds.
#include "internal.h"

namespace {

constexpr int NMS_THREADS = 256;          // steps 1: threads per workgroup (a thread per (n, b))
constexpr int NMS_SCAN_THREADS = 1024;    // the one-workgroup scan of the workgroup counts
constexpr int NMS_RESOLVE_THREADS = 1024; // step 2: 16 waves, a word of `alive` per wave at a time (a thread owns several words above NMS_RESOLVE_THREADS * 64 boxes)
constexpr int NMS_ORDER_THREADS = 1024;   // step 3
constexpr int NMS_MAX_WAVES = 16;
constexpr int64_t NMS_MAX_BOXES = (int64_t)1 << 30;

// f32::total_cmp as an unsigned key, ascending: -NaN < -Inf < ... < -0 < +0 < ... < +Inf < +NaN
__device__ __forceinline__ uint32_t total_key(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float nms_area(float t, float l, float b, float r) { return fmaxf(b - t, 0.f) * fmaxf(r - l, 0.f); }
__device__ __forceinline__ float nms_iou(float t, float l, float b, float r, float ot, float ol, float ob, float orr) {
    const float inter = nms_area(fmaxf(t, ot), fmaxf(l, ol), fminf(b, ob), fminf(r, orr));
    const float hull = nms_area(fminf(t, ot), fminf(l, ol), fmaxf(b, ob), fmaxf(r, orr));
    return inter / hull;
}

// Exclusive scan of one int per thread over the workgroup (blockDim.x a multiple of 64, at most 1024); every thread calls it.  lds: NMS_MAX_WAVES ints.
__device__ __forceinline__ int block_exclusive_scan(int v, int *lds, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    __syncthreads(); // the previous use of lds is over
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < waves; k++) {
        const int s = lds[k];
        if (k < wave) base += s;
        tot += s;
    }
    total = tot;
    return base + inc - v;
}

__global__ __launch_bounds__(NMS_THREADS) void nms_class_kernel(int64_t nb, int64_t B, int64_t C, float score_thr, const float *__restrict__ scores, float *__restrict__ st_score,
                                                               int32_t *__restrict__ st_cls, int32_t *__restrict__ blk_cnt) {
    const int64_t i = (int64_t)blockIdx.x * NMS_THREADS + threadIdx.x;
    int pass = 0;
    if (i < nb) {
        const int64_t n = i / B, b = i - n * B;
        const float *s = scores + n * C * B + b;
        float best = s[0];
        uint32_t best_key = total_key(best);
        int32_t cls = 0;
#pragma unroll 4
        for (int64_t c = 1; c < C; c++) {
            const float v = s[c * B];
            const uint32_t k = total_key(v);
            if (k >= best_key) { best_key = k; best = v; cls = (int32_t)c; } // Iterator::max_by: the last maximal element
        }
        pass = !(best < score_thr);
        st_score[i] = best;
        st_cls[i] = pass ? cls : -1;
    }
    const int cnt = __syncthreads_count(pass);
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(NMS_SCAN_THREADS) void nms_offsets_kernel(int64_t blocks, const int32_t *__restrict__ blk_cnt, int32_t *__restrict__ blk_off, int32_t *__restrict__ meta) {
    __shared__ int lds[NMS_MAX_WAVES];
    int base = 0;
    for (int64_t c0 = 0; c0 < blocks; c0 += NMS_SCAN_THREADS) {
        const int64_t k = c0 + threadIdx.x;
        const int v = k < blocks ? blk_cnt[k] : 0;
        int total;
        const int off = block_exclusive_scan(v, lds, total);
        if (k < blocks) blk_off[k] = base + off;
        base += total;
    }
    if (threadIdx.x == 0) meta[0] = base;
}

__global__ __launch_bounds__(NMS_THREADS) void nms_gather_kernel(int center, int64_t nb, const float *__restrict__ boxes, const float *__restrict__ st_score, const int32_t *__restrict__ st_cls,
                                                                const int32_t *__restrict__ blk_off, float *__restrict__ ct, float *__restrict__ cl, float *__restrict__ cb,
                                                                float *__restrict__ cr, float *__restrict__ cs, int32_t *__restrict__ ccls, int32_t *__restrict__ cpos) {
    __shared__ int lds[NMS_MAX_WAVES];
    const int64_t i = (int64_t)blockIdx.x * NMS_THREADS + threadIdx.x;
    const int32_t cls = i < nb ? st_cls[i] : -1;
    int total;
    const int rank = block_exclusive_scan(cls >= 0 ? 1 : 0, lds, total);
    if (cls < 0) return;
    const int64_t at = (int64_t)blk_off[blockIdx.x] + rank; // < the number of candidates <= nb
    const float c0 = boxes[4 * i], c1 = boxes[4 * i + 1], c2 = boxes[4 * i + 2], c3 = boxes[4 * i + 3]; // (any 4-byte alignment)
    float t = c0, l = c1, b = c2, r = c3;
    if (center) { // [cx, cy, w, h]
        const float hw = c2 / 2.f, hh = c3 / 2.f;
        t = c1 - hh; l = c0 - hw; b = c1 + hh; r = c0 + hw;
    }
    ct[at] = t; cl[at] = l; cb[at] = b; cr[at] = r;
    cs[at] = st_score[i];
    ccls[at] = cls;
    cpos[at] = (int32_t)i;
}

__global__ __launch_bounds__(NMS_RESOLVE_THREADS) void nms_resolve_kernel(float iou_thr, const float *__restrict__ ct, const float *__restrict__ cl, const float *__restrict__ cb,
                                                                         const float *__restrict__ cr, const float *__restrict__ cs, unsigned long long *__restrict__ alive,
                                                                         unsigned long long *__restrict__ removable, unsigned long long *__restrict__ keys, int32_t *__restrict__ meta) {
    __shared__ int red[2][NMS_MAX_WAVES];
    __shared__ int lds[NMS_MAX_WAVES];
    constexpr int T = NMS_RESOLVE_THREADS, WAVES = T / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = meta[0];
    const int words = (M + 63) >> 6;
    // word w belongs to wave w % WAVES, and there to lane (w / WAVES) % 64: only that thread ever reads or writes alive[w]
    for (int w = wave + WAVES * lane; w < words; w += WAVES * 64) alive[w] = 0ull;
    for (int p = 0; p < M; p++) {
        const float pt = ct[p], pl = cl[p], pb = cb[p], pr = cr[p], ps = cs[p];
        const int nw = (p + 63) >> 6; // the words that hold a q < p (bits at and above p are still 0)
        int j = INT32_MAX;
        unsigned long long mine0 = 0ull, rem0 = 0ull; // this thread's word of the first block, and what p removes from it
        for (int kb = 0; wave + WAVES * kb < nw && j == INT32_MAX; kb += 64) { // 64 of the wave's words at a time, a lane per word
            const int wk = wave + WAVES * (kb + lane);
            const unsigned long long mine = wk < nw ? alive[wk] : 0ull;
            if (kb == 0) mine0 = mine;
            unsigned long long nonzero = __ballot(mine != 0ull);
            int most = __popcll(mine);
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) most = max(most, __shfl_xor(most, d, 64));
            if (most <= __popcll(nonzero)) {
                // few members per word (rounds = the fullest word's members, fewer than the words that have any): every lane walks its own word
                unsigned long long a = mine, rm = 0ull;
                int jl = INT32_MAX;
                while (a) {
                    const int bit = __ffsll((long long)a) - 1;
                    a &= a - 1;
                    const int q = (wk << 6) + bit;
                    const float iou = nms_iou(pt, pl, pb, pr, ct[q], cl[q], cb[q], cr[q]);
                    if (iou >= iou_thr) {
                        if (ps > cs[q]) rm |= 1ull << bit;
                        else { jl = q; break; } // this word's first blocker: rm holds what lies below it
                    }
                }
                int jw = jl;
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) jw = min(jw, __shfl_xor(jw, d, 64));
                j = jw; // (words above the blocker's are not applied, whatever their rm)
                if (kb == 0) rem0 = rm;
                else if (mine) removable[wk] = rm;
                continue;
            }
            while (nonzero) { // the words with a member, in ascending order; the wave takes one at a time, a lane per member
                const int k = __ffsll((long long)nonzero) - 1;
                nonzero &= nonzero - 1;
                const unsigned lo = (unsigned)__shfl((int)(unsigned)(mine & 0xffffffffull), k, 64), hi = (unsigned)__shfl((int)(unsigned)(mine >> 32), k, 64);
                const unsigned long long a = ((unsigned long long)hi << 32) | lo;
                const int w = wave + WAVES * (kb + k), q = (w << 6) + lane;
                bool blocks = false, removes = false;
                if ((a >> lane) & 1ull) {
                    const float iou = nms_iou(pt, pl, pb, pr, ct[q], cl[q], cb[q], cr[q]);
                    if (iou >= iou_thr) {
                        if (ps > cs[q]) removes = true;
                        else blocks = true;
                    }
                }
                const unsigned long long blk = __ballot(blocks);
                unsigned long long rm = __ballot(removes);
                if (blk) { // the wave's first blocker: nothing at or above it can be removed, and its later words do not matter
                    const int bit = __ffsll((long long)blk) - 1;
                    j = (w << 6) + bit;
                    rm &= (1ull << bit) - 1ull;
                }
                if (kb == 0) { if (lane == k) rem0 = rm; }
                else if (lane == 0) removable[w] = rm; // (beyond 64 words per wave: through memory, read back by the word's owner after the barrier)
                if (blk) break;
            }
        }
        if (lane == 0) red[p & 1][wave] = j; // (j is the same in every lane of the wave)
        __syncthreads(); // the only barrier of a candidate: the next one writes the other set of slots
        int first = INT32_MAX;
#pragma unroll
        for (int k = 0; k < WAVES; k++) first = min(first, red[p & 1][k]);
        // A wave that stopped at its own blocker jw >= first has dealt with every word of its own up to jw's: with every word below `first`.
        {
            const int wk = wave + WAVES * lane;
            if (wk < nw && (first == INT32_MAX || (wk << 6) < first)) {
                unsigned long long rm = rem0;
                if (first != INT32_MAX && (first >> 6) == wk) rm &= (1ull << (first & 63)) - 1ull;
                if (rm & mine0) alive[wk] = mine0 & ~rm;
            }
        }
        for (int kb = 64; wave + WAVES * kb < nw; kb += 64) {
            const int wk = wave + WAVES * (kb + lane);
            if (wk < nw && (first == INT32_MAX || (wk << 6) < first)) {
                const unsigned long long mine = alive[wk];
                if (mine) { // (a word without members was not visited: its `removable` is stale, and there is nothing to remove)
                    unsigned long long rm = removable[wk];
                    if (first != INT32_MAX && (first >> 6) == wk) rm &= (1ull << (first & 63)) - 1ull;
                    if (rm & mine) alive[wk] = mine & ~rm;
                }
            }
        }
        if (first == INT32_MAX) {
            const int w = p >> 6;
            if (w % WAVES == wave && (w / WAVES) % 64 == lane) alive[w] |= 1ull << (p & 63);
        }
    }
    __syncthreads();
    // the survivors in candidate order, as sort keys
    int base = 0;
    for (int w0 = 0; w0 < words; w0 += T) {
        const int w = w0 + tid; // (read by another thread than the word's owner: the barrier above orders it)
        unsigned long long a = w < words ? alive[w] : 0ull;
        int total;
        int at = base + block_exclusive_scan(__popcll(a), lds, total);
        while (a) {
            const int bit = __ffsll((long long)a) - 1;
            a &= a - 1;
            const int q = (w << 6) + bit;
            keys[at++] = ((unsigned long long)(~total_key(cs[q])) << 32) | (unsigned)q;
        }
        base += total;
    }
    if (tid == 0) meta[1] = base;
}

__global__ __launch_bounds__(NMS_ORDER_THREADS) void nms_order_kernel(int has_cap, int cap, int64_t B, int64_t C, const int32_t *__restrict__ ccls, const int32_t *__restrict__ cpos,
                                                                     unsigned long long *__restrict__ keys, int32_t *__restrict__ cls_count, int32_t *__restrict__ out,
                                                                     int32_t *__restrict__ meta) {
    __shared__ int lds[NMS_MAX_WAVES];
    __shared__ int chunk_cls[NMS_ORDER_THREADS];
    const int tid = threadIdx.x;
    const int S = meta[1];
    if (S == 0 || (has_cap && cap <= 0)) { // (uniform)
        if (tid == 0) meta[2] = 0;
        return;
    }
    int P = 1;
    while (P < S) P <<= 1; // <= the capacity of keys (the next power of two of N * B)
    for (int i = S + tid; i < P; i += NMS_ORDER_THREADS) keys[i] = ~0ull;
    if (has_cap) for (int64_t c = tid; c < C; c += NMS_ORDER_THREADS) cls_count[c] = 0;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += NMS_ORDER_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = keys[i], b = keys[l];
                    if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
                }
            }
            __syncthreads();
        }
    int base = 0;
    for (int c0 = 0; c0 < S; c0 += NMS_ORDER_THREADS) {
        const int i = c0 + tid;
        const bool valid = i < S;
        const int q = valid ? (int)(unsigned)(keys[i] & 0xffffffffull) : 0;
        const int cls = valid ? ccls[q] : -1;
        int keep = valid ? 1 : 0;
        if (has_cap) {
            chunk_cls[tid] = cls;
            __syncthreads();
            int earlier = 0;
            bool later = false;
            if (valid)
                for (int k = 0; k < NMS_ORDER_THREADS; k++) {
                    const bool same = chunk_cls[k] == cls;
                    earlier += (same && k < tid) ? 1 : 0;
                    later = later || (same && k > tid);
                }
            const int rank = valid ? cls_count[cls] + earlier : 0;
            keep = valid && rank < cap;
            __syncthreads(); // every read of cls_count and chunk_cls is done
            if (valid && !later) cls_count[cls] = rank + 1; // the class's last row of the chunk carries its count on
        }
        int total;
        const int at = base + block_exclusive_scan(keep, lds, total); // (its barriers also order cls_count for the next chunk)
        if (keep) {
            const int64_t pos = cpos[q];
            const int64_t n = pos / B;
            out[3 * (int64_t)at + 0] = (int32_t)n;
            out[3 * (int64_t)at + 1] = cls;
            out[3 * (int64_t)at + 2] = (int32_t)(pos - n * B);
        }
        base += total;
    }
    if (tid == 0) meta[2] = base;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

} // namespace

RTEN_EXPORT int32_t rten_hip_non_max_suppression_f32(rten_hip_ctx *ctx, int32_t center_point_box, int64_t n, int64_t c, int64_t b, const float *boxes, const float *scores,
                                                     int32_t has_max_per_class, int32_t max_per_class, float iou_threshold, float score_threshold, int32_t *selected,
                                                     int64_t *count) {
    RTEN_CHECK_CTX(ctx);
    // the count is read back: refused before anything is launched or copied
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (ctx->capturing || (hipStreamIsCapturing(ctx->stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone))
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "non_max_suppression: the row count is read back from the device, so the call cannot be captured into a graph");
    if (!count) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "non_max_suppression: null count");
    if (center_point_box != 0 && center_point_box != 1) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "non_max_suppression: center_point_box is 0 or 1");
    if (n < 0 || c < 0 || b < 0 || n > NMS_MAX_BOXES || b > NMS_MAX_BOXES || c > 0x7fffffff || (double)n * (double)b > (double)NMS_MAX_BOXES ||
        (double)n * (double)b * (double)c >= 9.0e18)
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "non_max_suppression: bad dimension");
    *count = 0;
    const int64_t nb = n * b;
    if (nb == 0 || c == 0) return RTEN_HIP_OK;
    if (!boxes || !scores || !selected) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "non_max_suppression: null input or output");

    const int64_t blocks = ceil_div64(nb, NMS_THREADS), words = ceil_div64(nb, 64);
    int64_t pow2 = 1;
    while (pow2 < nb) pow2 <<= 1;
    // scratch: every size from N * B and C
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off += align256(bytes); return at; };
    const size_t o_meta = take(4 * 4), o_sts = take(4 * (size_t)nb), o_stc = take(4 * (size_t)nb), o_bcnt = take(4 * (size_t)blocks), o_boff = take(4 * (size_t)blocks);
    const size_t o_t = take(4 * (size_t)nb), o_l = take(4 * (size_t)nb), o_b = take(4 * (size_t)nb), o_r = take(4 * (size_t)nb), o_s = take(4 * (size_t)nb);
    const size_t o_cls = take(4 * (size_t)nb), o_pos = take(4 * (size_t)nb), o_alive = take(8 * (size_t)words), o_rem = take(8 * (size_t)words), o_keys = take(8 * (size_t)pow2);
    const size_t o_ccnt = take(has_max_per_class ? 4 * (size_t)c : 0);
    char *base = (char *)rten_aux_scratch(ctx, off);
    if (!base) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "non_max_suppression: no scratch memory (%zu bytes)", off);
    int32_t *meta = (int32_t *)(base + o_meta), *st_cls = (int32_t *)(base + o_stc), *blk_cnt = (int32_t *)(base + o_bcnt), *blk_off = (int32_t *)(base + o_boff);
    float *st_score = (float *)(base + o_sts), *ct = (float *)(base + o_t), *cl = (float *)(base + o_l), *cb = (float *)(base + o_b), *cr = (float *)(base + o_r), *cs = (float *)(base + o_s);
    int32_t *ccls = (int32_t *)(base + o_cls), *cpos = (int32_t *)(base + o_pos), *cls_count = (int32_t *)(base + o_ccnt);
    unsigned long long *alive = (unsigned long long *)(base + o_alive), *removable = (unsigned long long *)(base + o_rem), *keys = (unsigned long long *)(base + o_keys);

    {
        ProfScope ps(ctx, "nms_class_f32", 0.0, 4.0 * nb * c + 8.0 * nb);
        hipLaunchKernelGGL(nms_class_kernel, dim3((unsigned)blocks), dim3(NMS_THREADS), 0, ctx->stream, nb, b, c, score_threshold, scores, st_score, st_cls, blk_cnt);
    }
    RTEN_LAUNCH_CHECK(ctx, "nms_class_f32");
    {
        ProfScope ps(ctx, "nms_offsets", 0.0, 8.0 * blocks);
        hipLaunchKernelGGL(nms_offsets_kernel, dim3(1), dim3(NMS_SCAN_THREADS), 0, ctx->stream, blocks, blk_cnt, blk_off, meta);
    }
    RTEN_LAUNCH_CHECK(ctx, "nms_offsets");
    {
        ProfScope ps(ctx, "nms_gather_f32", 0.0, 52.0 * nb);
        hipLaunchKernelGGL(nms_gather_kernel, dim3((unsigned)blocks), dim3(NMS_THREADS), 0, ctx->stream, center_point_box, nb, boxes, st_score, st_cls, blk_off, ct, cl, cb, cr, cs, ccls, cpos);
    }
    RTEN_LAUNCH_CHECK(ctx, "nms_gather_f32");
    {
        ProfScope ps(ctx, "nms_resolve", 0.0, 0.0);
        hipLaunchKernelGGL(nms_resolve_kernel, dim3(1), dim3(NMS_RESOLVE_THREADS), 0, ctx->stream, iou_threshold, ct, cl, cb, cr, cs, alive,
                           removable, keys, meta);
    }
    RTEN_LAUNCH_CHECK(ctx, "nms_resolve");
    {
        ProfScope ps(ctx, "nms_order", 0.0, 0.0);
        hipLaunchKernelGGL(nms_order_kernel, dim3(1), dim3(NMS_ORDER_THREADS), 0, ctx->stream, has_max_per_class != 0, max_per_class, b, c, ccls, cpos, keys, cls_count, selected, meta);
    }
    RTEN_LAUNCH_CHECK(ctx, "nms_order");
    int32_t rows = 0;
    RTEN_HIP_TRY(ctx, hipMemcpyAsync(&rows, meta + 2, sizeof(rows), hipMemcpyDeviceToHost, ctx->stream));
    RTEN_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (const int32_t rc = rten_check_fault(ctx)) return rc;
    *count = rows;
    return RTEN_HIP_OK;
}
