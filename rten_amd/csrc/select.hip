// The selection family (src/ops/reduce.rs:64-215 ArgMax / ArgMin, :876-1044 ReduceMin / ReduceMax, :1236-1356 TopK) on strided views, float32 and int32.
//
// Every operator here is a MAXIMUM OVER UNSIGNED KEYS, so one set of reductions serves all of them and no comparison has a special case:
//   * an element becomes `ukey`: the order-preserving unsigned image of its value (f32: sign bit set for positives, all bits flipped for negatives;
//     int32: biased by 2^31), with every NaN -- whatever its sign or payload -- mapped to 0xffffffff, above +inf;
//   * ReduceMax reduces `ukey`, ReduceMin reduces `~ukey` with NaN still on top ("a NaN anywhere makes the result NaN", minimum_num / maximum_num); the
//     result is decoded back, a NaN as the canonical quiet NaN;
//   * ArgMax / ArgMin reduce the 64-bit key (that word, index word): Iterator::max_by with cmp_nan_greater keeps the FIRST NaN and otherwise the LAST of
//     equal extremes, so the index word is ~i under a NaN and i otherwise.  -0 and +0 compare equal in the reference: both get +0's key;
//   * TopK sorts 64-bit keys (value word, ~i) in descending order: "smaller index first among equal values, in both directions" is the ~i, "NaN greater than
//     everything regardless of `largest`" is NaN = 0xffffffff for largest and 0 for smallest (where the value word is ~ukey).  Values are gathered from the
//     input by the selected index, so they keep their bits (sign of zero, NaN payload).
// Nothing is packed: lanes are read through the view's strides.  No kernel uses scratch registers; every store is a vector store.
#include "internal.h"
#include "slice.h" // the kept / reduced levels and their addressing

namespace {

constexpr int WAVES_PER_BLOCK = 4;
constexpr unsigned NAN_KEY = 0xffffffffu;

struct SelArgs {
    SliceLevels<1> kept, red;
    int64_t rows;  // output elements (lanes)
    int inner;     // reduced slice length, < 2^31
    int chunk;     // two-pass form: elements per partial (a multiple of 4); otherwise == inner
    int nchunks;   // partials per row (1: the kernel writes the decoded result)
    unsigned flip; // 0: max, 0xffffffff: min (xor on the key of a number)
};

// ---- keys
// CANON: -0 takes +0's key (operators whose comparison says the two are equal).  ReduceMax / ReduceMin keep them apart (-0 < +0): either zero is right
// there, and this way the zero returned is one that occurs in the slice.
template <int DT, bool CANON>
__device__ __forceinline__ unsigned ukey_of(unsigned b) {
    if (DT == RTEN_HIP_DT_I32) return b ^ 0x80000000u;
    if ((b & 0x7fffffffu) > 0x7f800000u) return NAN_KEY;
    if (CANON && b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
template <int DT>
__device__ __forceinline__ unsigned bits_of_ukey(unsigned u) {
    if (DT == RTEN_HIP_DT_I32) return u ^ 0x80000000u;
    return (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
}

// One reduction state per key width.  K32: ReduceMax / ReduceMin.  K64: ArgMax / ArgMin.
template <int DT>
struct K32 {
    typedef unsigned T;
    static __device__ __forceinline__ T identity() { return 0; }
    static __device__ __forceinline__ T make(unsigned bits, int, unsigned flip) {
        const unsigned u = ukey_of<DT, false>(bits);
        return (DT == RTEN_HIP_DT_F32 && u == NAN_KEY) ? u : (u ^ flip);
    }
    static __device__ __forceinline__ unsigned decode(T k, unsigned flip) {
        if (DT == RTEN_HIP_DT_F32 && k == NAN_KEY) return 0x7fc00000u; // (no number has this key in either direction: ~ukey(-inf) = 0xff7fffff)
        return bits_of_ukey<DT>(k ^ flip);
    }
};
template <int DT>
struct K64 {
    typedef unsigned long long T;
    static __device__ __forceinline__ T identity() { return 0; }
    static __device__ __forceinline__ T make(unsigned bits, int i, unsigned flip) {
        const unsigned u = ukey_of<DT, true>(bits);
        const bool nan = DT == RTEN_HIP_DT_F32 && u == NAN_KEY;
        return ((T)(nan ? u : (u ^ flip)) << 32) | (unsigned)(nan ? ~i : i);
    }
    static __device__ __forceinline__ unsigned decode(T k, unsigned) {
        const bool nan = DT == RTEN_HIP_DT_F32 && (unsigned)(k >> 32) == NAN_KEY;
        return nan ? ~(unsigned)k : (unsigned)k;
    }
};

__device__ __forceinline__ unsigned kmax(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long kmax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// rotate within each 16-lane DPP row (row_ror:N): the cross-lane step of a butterfly whose operator commutes
template <int N>
__device__ __forceinline__ unsigned row_ror(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x120 + N, 0xf, 0xf, false); }
template <int N>
__device__ __forceinline__ unsigned long long row_ror(unsigned long long v) {
    return ((unsigned long long)row_ror<N>((unsigned)(v >> 32)) << 32) | row_ror<N>((unsigned)v);
}
__device__ __forceinline__ unsigned xor_lane(unsigned v, int m) { return (unsigned)__shfl_xor((int)v, m, 64); }
__device__ __forceinline__ unsigned long long xor_lane(unsigned long long v, int m) {
    return ((unsigned long long)xor_lane((unsigned)(v >> 32), m) << 32) | xor_lane((unsigned)v, m);
}
// maximum over the LPR (16 or 64) lanes of a row group, left in every lane of the group
template <int LPR, typename T>
__device__ __forceinline__ T group_max(T v) {
    v = kmax(v, row_ror<8>(v));
    v = kmax(v, row_ror<4>(v));
    v = kmax(v, row_ror<2>(v));
    v = kmax(v, row_ror<1>(v));
    if (LPR == 64) {
        v = kmax(v, xor_lane(v, 16));
        v = kmax(v, xor_lane(v, 32));
    }
    return v;
}

// ---- reduced axes walked by the lanes of a wave: LPR = 64, one (row, chunk) per wave; LPR = 16, four per wave on the DPP rows (slices of <= 256).
// VEC: the slice is contiguous and every row base is 16-byte aligned -> dwordx4 loads.  With nchunks > 1 the raw keys go to `part` and
// select_finish_kernel folds them (the whole-tensor reduction: a row's chunks are spread over the machine instead of one wave crawling it).
template <class KT, int LPR, bool VEC>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void select_rows_kernel(const SelArgs p, const unsigned *__restrict__ x, unsigned *__restrict__ y,
                                                                           typename KT::T *__restrict__ part) {
    typedef typename KT::T T;
    constexpr int GROUPS = 64 / LPR;
    const int lane = threadIdx.x & 63, l = lane & (LPR - 1);
    const int64_t units = p.rows * p.nchunks;
    const int64_t unit = ((int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6)) * GROUPS + (GROUPS > 1 ? lane / LPR : 0);
    const int64_t uu = unit < units ? unit : units - 1; // (clamped, not returned: the row's lanes all take part in the DPP steps)
    const int64_t row = p.nchunks > 1 ? uu / p.nchunks : uu;
    const int c = p.nchunks > 1 ? (int)(uu - row * p.nchunks) : 0;
    const int i0 = c * p.chunk, i1 = (p.inner - i0 < p.chunk) ? p.inner : i0 + p.chunk;
    const unsigned *xr = x + slice_row_base(p.kept, p.rows, row);
    T acc = KT::identity();
    if (VEC) {
        const int v1 = i0 + ((i1 - i0) & ~3);
        auto fold = [&](const uint4 &v, int i) {
            acc = kmax(acc, KT::make(v.x, i, p.flip));
            acc = kmax(acc, KT::make(v.y, i + 1, p.flip));
            acc = kmax(acc, KT::make(v.z, i + 2, p.flip));
            acc = kmax(acc, KT::make(v.w, i + 3, p.flip));
        };
        int i = i0 + 4 * l;
        for (; i + 12 * LPR < v1; i += 16 * LPR) { // four independent 16-byte loads in flight per lane
            uint4 v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = *reinterpret_cast<const uint4 *>(xr + i + 4 * LPR * q);
#pragma unroll
            for (int q = 0; q < 4; q++) fold(v[q], i + 4 * LPR * q);
        }
        if (i + 4 * LPR < v1) { // two
            const uint4 a = *reinterpret_cast<const uint4 *>(xr + i), b = *reinterpret_cast<const uint4 *>(xr + i + 4 * LPR);
            fold(a, i);
            fold(b, i + 4 * LPR);
            i += 8 * LPR;
        }
        for (; i < v1; i += 4 * LPR) fold(*reinterpret_cast<const uint4 *>(xr + i), i);
        if (v1 + l < i1 && l < 3) acc = kmax(acc, KT::make(xr[v1 + l], v1 + l, p.flip));
    } else {
        int i = i0 + l;
        for (; i + 3 * LPR < i1; i += 4 * LPR) { // four independent loads in flight per lane
            unsigned v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = xr[slice_elem_off(p.red, i + q * LPR)];
#pragma unroll
            for (int q = 0; q < 4; q++) acc = kmax(acc, KT::make(v[q], i + q * LPR, p.flip));
        }
        for (; i < i1; i += LPR) acc = kmax(acc, KT::make(xr[slice_elem_off(p.red, i)], i, p.flip));
    }
    acc = group_max<LPR>(acc);
    if (l == 0 && unit < units) {
        if (p.nchunks > 1) part[unit] = acc;
        else y[row] = KT::decode(acc, p.flip);
    }
}

// second launch of the two-pass form: one wave per row folds its partial keys
template <class KT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void select_finish_kernel(int64_t rows, int nchunks, unsigned flip, const typename KT::T *__restrict__ part,
                                                                             unsigned *__restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    typename KT::T acc = KT::identity();
    for (int i = lane; i < nchunks; i += 64) acc = kmax(acc, part[row * nchunks + i]);
    acc = group_max<64>(acc);
    if (lane == 0) y[row] = KT::decode(acc, flip);
}

// ---- reduced axes strided, innermost kept axis contiguous (ArgMax / ReduceMax over the channels of [N, C, H, W], a column maximum): lanes run along the
// kept axis, so every load is coalesced, and the reduced axes are a loop.  A workgroup owns `cw` adjacent outputs (a power of two <= its size); its
// blockDim / cw thread groups take the slice elements s, s + split, ... and meet in LDS.  split == 1 (a short slice, many outputs): no cross-lane step at all.
template <class KT>
__global__ __launch_bounds__(1024) void select_cols_kernel(const SelArgs p, int cw, const unsigned *__restrict__ x, unsigned *__restrict__ y) {
    typedef typename KT::T T;
    __shared__ T part[1024];
    const int last = p.kept.shape[p.kept.n - 1];
    const int groups = (last + cw - 1) / cw;
    const int split = (int)blockDim.x / cw;
    const int j = threadIdx.x & (cw - 1), s = threadIdx.x / cw;
    // Neighbouring column groups narrower than a 128-byte line read parts of the same lines.  Workgroup ids go round-robin over the eight XCDs, so neighbours
    // in id order never share an L2; here each XCD gets a CONTIGUOUS run of groups (ids id, id + 8, ... are dispatched to the same XCD one after the other).
    unsigned bid = blockIdx.x;
    if (cw < 32) {
        const unsigned nt = gridDim.x, xcd = bid & 7, qn = nt >> 3, rn = nt & 7;
        bid = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + (bid >> 3);
    }
    const int64_t prefix = bid / groups;
    const int j0 = (int)(bid - prefix * groups) * cw;
    const bool live = j0 + j < last;
    const int64_t row = prefix * last + (live ? j0 + j : last - 1);
    const unsigned *xr = x + slice_row_base(p.kept, p.rows, row);
    T acc = KT::identity();
    int i = s;
    for (; i + 15 * split < p.inner; i += 16 * split) { // sixteen independent loads in flight per lane
        unsigned v[16];
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] = xr[slice_elem_off(p.red, i + q * split)];
#pragma unroll
        for (int q = 0; q < 16; q++) acc = kmax(acc, KT::make(v[q], i + q * split, p.flip));
    }
    for (; i + 3 * split < p.inner; i += 4 * split) {
        unsigned v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = xr[slice_elem_off(p.red, i + q * split)];
#pragma unroll
        for (int q = 0; q < 4; q++) acc = kmax(acc, KT::make(v[q], i + q * split, p.flip));
    }
    for (; i < p.inner; i += split) acc = kmax(acc, KT::make(xr[slice_elem_off(p.red, i)], i, p.flip));
    if (split > 1 && cw < 64) { // the thread groups of one wave meet in registers, the waves (at most 16) in LDS
        for (int m = cw; m < 64; m <<= 1) acc = kmax(acc, xor_lane(acc, m));
        const int wave = threadIdx.x >> 6, waves = (int)blockDim.x >> 6;
        if ((threadIdx.x & 63) < cw) part[wave * cw + j] = acc;
        __syncthreads();
        if (s == 0)
            for (int q = 1; q < waves; q++) acc = kmax(acc, part[q * cw + j]);
    } else if (split > 1) { // whole waves per thread group: at most 16 groups
        part[threadIdx.x] = acc;
        __syncthreads();
        if (s == 0)
            for (int q = 1; q < split; q++) acc = kmax(acc, part[q * cw + j]);
    }
    if (s == 0 && live) y[row] = KT::decode(acc, p.flip);
}

// ---- TopK: the k largest 64-bit keys of a lane in descending order.  One workgroup sorts up to P (a power of two, 128..8192) keys in LDS with a bitonic network.
// A lane of at most P elements is one launch.  A longer lane is cut into chunks of P whose first kk = min(k, P) keys go to a list in global memory
// (padded with key 0, below every real key since the index word ~i of a real key is >= 2^31); merge launches then sort `per` lists at a time until one is left.
struct TopkArgs {
    SliceLevels<2> kept;  // stride lists: 0 the input's, 1 the outputs'
    int64_t lanes;
    int axis_len;
    int64_t axis_stride;  // of the input, in elements
    int k;
    int P;                // keys sorted per workgroup
    int units;            // workgroups per lane in this launch
    int from_lists;       // 0: keys come from the input's chunk `unit`; 1: from lists [unit * per, ...) of the previous launch
    int per, nlists, kk;  // lists merged per workgroup / lists per lane on input / keys per list
    int final;            // 1: write values and indices; 0: write a list of kk keys
    unsigned vflip;       // 0: largest, 0xffffffff: smallest
    int64_t out_axis_stride;
};

template <int DT>
__global__ __launch_bounds__(1024) void topk_sort_kernel(const TopkArgs p, const unsigned *__restrict__ x, const unsigned long long *__restrict__ lists_in,
                                                         unsigned long long *__restrict__ lists_out, unsigned *__restrict__ values, int32_t *__restrict__ indices) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    const int64_t lane_id = blockIdx.x / p.units;
    const int unit = (int)(blockIdx.x - lane_id * p.units);
    int64_t base[2]; // of the lane in the input, in the outputs
    slice_row_bases(p.kept, p.lanes, lane_id, base);
    const int64_t out_off = base[1];
    const unsigned *xl = x + base[0];
    if (!p.from_lists) {
        const int64_t i0 = (int64_t)unit * p.P;
        for (int t = threadIdx.x; t < p.P; t += blockDim.x) {
            const int64_t i = i0 + t;
            unsigned long long key = 0;
            if (i < p.axis_len) {
                const unsigned u = ukey_of<DT, true>(xl[i * p.axis_stride]);
                const unsigned w = (DT == RTEN_HIP_DT_F32 && u == NAN_KEY) ? ~p.vflip : (u ^ p.vflip); // NaN: first for largest, last for smallest
                key = ((unsigned long long)w << 32) | (unsigned)~(unsigned)i;
            }
            keys[t] = key;
        }
    } else {
        const int l0 = unit * p.per;
        const int n = (p.nlists - l0 < p.per ? p.nlists - l0 : p.per) * p.kk;
        const unsigned long long *src = lists_in + ((int64_t)lane_id * p.nlists + l0) * p.kk;
        for (int t = threadIdx.x; t < p.P; t += blockDim.x) keys[t] = t < n ? src[t] : 0ull;
    }
    __syncthreads();
    for (int size = 2; size <= p.P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (p.P >> 1); t += blockDim.x) {
                const int a = 2 * t - (t & (stride - 1)), b = a + stride;
                const unsigned long long ka = keys[a], kb = keys[b];
                const bool desc = (a & size) == 0;
                if (desc ? ka < kb : ka > kb) {
                    keys[a] = kb;
                    keys[b] = ka;
                }
            }
            __syncthreads();
        }
    }
    if (p.final) {
        for (int t = threadIdx.x; t < p.k; t += blockDim.x) {
            const unsigned i = ~(unsigned)keys[t];
            values[out_off + t * p.out_axis_stride] = xl[(int64_t)i * p.axis_stride];
            indices[out_off + t * p.out_axis_stride] = (int32_t)i;
        }
    } else {
        unsigned long long *dst = lists_out + ((int64_t)lane_id * p.units + unit) * p.kk;
        for (int t = threadIdx.x; t < p.kk; t += blockDim.x) dst[t] = keys[t];
    }
}

int next_pow2(int64_t v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// the checks ReduceMax / ReduceMin and ArgMax / ArgMin share, in their order; fills `p` (without chunking)
int32_t select_args(rten_hip_ctx *ctx, const char *what, SelArgs &p, int32_t op, int32_t dtype, int32_t n_outer, const int64_t *outer_shape,
                    const int64_t *outer_strides, int32_t n_inner, const int64_t *inner_shape, const int64_t *inner_strides) {
    if (op != RTEN_HIP_SELECT_MAX && op != RTEN_HIP_SELECT_MIN) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "%s: op must be RTEN_HIP_SELECT_MAX or _MIN", what);
    if (dtype != RTEN_HIP_DT_F32 && dtype != RTEN_HIP_DT_I32) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "%s: element type must be float32 or int32", what);
    p = SelArgs{};
    if (int32_t rc = slice_fill(ctx, what, n_outer, outer_shape, {outer_strides}, p.kept, p.rows, n_inner, inner_shape, inner_strides, &p.red, &p.inner)) return rc;
    p.flip = op == RTEN_HIP_SELECT_MIN ? 0xffffffffu : 0u;
    p.chunk = p.inner;
    p.nchunks = 1;
    return RTEN_HIP_OK;
}

// the launch plan shared by ReduceMax / ReduceMin (KT = K32) and ArgMax / ArgMin (KT = K64); p.inner > 0, p.rows > 0
template <class KT>
int32_t launch_select(rten_hip_ctx *ctx, SelArgs p, const void *xv, void *yv) {
    typedef typename KT::T T;
    const unsigned *x = (const unsigned *)xv;
    unsigned *y = (unsigned *)yv;
    const int64_t last = p.kept.n ? p.kept.shape[p.kept.n - 1] : 1;
    if (p.kept.n && p.kept.stride[0][p.kept.n - 1] == 1 && last >= 16 && p.red.stride[0][p.red.n - 1] > 1 && p.rows / last * ((last + 63) / 64) <= 0x7fffffff) {
        // thread per output while the outputs alone fill the machine or the slice is short; otherwise the slice is split over the workgroup's thread groups
        const bool flat = p.inner < 64 || p.rows >= (int64_t)64 * 16 * ctx->num_cus;
        const int block = flat ? 256 : 1024;
        const int cw = flat ? (last >= 256 ? 256 : next_pow2(last)) : (p.rows / last * ((last + 63) / 64) >= 2 * ctx->num_cus ? 64 : 16);
        const int64_t grid = p.rows / last * ((last + cw - 1) / cw);
        hipLaunchKernelGGL(select_cols_kernel<KT>, dim3((unsigned)grid), dim3(block), 0, ctx->stream, p, cw, x, y);
        RTEN_LAUNCH_CHECK(ctx, "select_cols_kernel");
        return RTEN_HIP_OK;
    }
    bool vec = p.red.n == 1 && p.red.stride[0][0] == 1 && ((uintptr_t)x & 15) == 0;
    for (int d = 0; d < p.kept.n; d++) vec = vec && (p.kept.stride[0][d] & 3) == 0;
    // few rows, long slices: partials first, so that the machine (not rows * 64 lanes) reads the tensor
    T *part = nullptr;
    if (p.rows < (int64_t)8 * ctx->num_cus && p.inner >= 16384) {
        int64_t want = ((int64_t)16 * ctx->num_cus + p.rows - 1) / p.rows; // ~16 waves per compute unit in all
        if (want > 8192) want = 8192;
        int64_t chunk = (p.inner + want - 1) / want;
        if (chunk < 4096) chunk = 4096;
        chunk = (chunk + 3) & ~(int64_t)3;
        const int nchunks = (int)((p.inner + chunk - 1) / chunk);
        if (nchunks > 1) {
            part = (T *)rten_scratch(ctx, sizeof(T) * (size_t)(p.rows * nchunks));
            if (!part) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "select: no scratch for %lld partial keys", (long long)(p.rows * nchunks));
            p.chunk = (int)chunk;
            p.nchunks = nchunks;
        }
    }
    const int64_t units = p.rows * p.nchunks;
    const dim3 block(64 * WAVES_PER_BLOCK);
    const int64_t g64 = (units + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, g16 = (units + 4 * WAVES_PER_BLOCK - 1) / (4 * WAVES_PER_BLOCK);
    if (g64 > 0x7fffffff) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "select: more than 2^33 lanes");
    if (p.inner <= 256 && p.nchunks == 1) {
        if (vec) hipLaunchKernelGGL((select_rows_kernel<KT, 16, true>), dim3((unsigned)g16), block, 0, ctx->stream, p, x, y, part);
        else hipLaunchKernelGGL((select_rows_kernel<KT, 16, false>), dim3((unsigned)g16), block, 0, ctx->stream, p, x, y, part);
    } else {
        if (vec) hipLaunchKernelGGL((select_rows_kernel<KT, 64, true>), dim3((unsigned)g64), block, 0, ctx->stream, p, x, y, part);
        else hipLaunchKernelGGL((select_rows_kernel<KT, 64, false>), dim3((unsigned)g64), block, 0, ctx->stream, p, x, y, part);
    }
    RTEN_LAUNCH_CHECK(ctx, "select_rows_kernel");
    if (p.nchunks > 1) {
        hipLaunchKernelGGL(select_finish_kernel<KT>, dim3((unsigned)((p.rows + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK)), block, 0, ctx->stream, p.rows, p.nchunks, p.flip, part, y);
        RTEN_LAUNCH_CHECK(ctx, "select_finish_kernel");
    }
    return RTEN_HIP_OK;
}

} // namespace

RTEN_EXPORT int32_t rten_hip_reduce_minmax_strided(rten_hip_ctx *ctx, int32_t op, int32_t dtype, int32_t n_outer, const int64_t *outer_shape,
                                                   const int64_t *outer_strides, int32_t n_inner, const int64_t *inner_shape, const int64_t *inner_strides,
                                                   const void *x, void *y) {
    RTEN_CHECK_CTX(ctx);
    SelArgs p;
    if (int32_t rc = select_args(ctx, "reduce_minmax", p, op, dtype, n_outer, outer_shape, outer_strides, n_inner, inner_shape, inner_strides)) return rc;
    if (p.rows == 0) return RTEN_HIP_OK;
    if (!y) return RTEN_HIP_ERR_INVALID_VALUE;
    if (p.inner == 0) { // an empty slice gives the kernel's identity (reduce.rs:446-452; slice_fold_assoc's initial value / MaxNum's -inf)
        const bool mx = op == RTEN_HIP_SELECT_MAX;
        const unsigned ident = dtype == RTEN_HIP_DT_F32 ? (mx ? 0xff800000u : 0x7f800000u) : (mx ? 0x80000000u : 0x7fffffffu);
        RTEN_HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)y, (int)ident, (size_t)p.rows, ctx->stream));
        return RTEN_HIP_OK;
    }
    if (!x) return RTEN_HIP_ERR_INVALID_VALUE;
    ProfScope ps(ctx, "reduce_minmax", 0.0, 4.0 * p.rows * ((double)p.inner + 1));
    return dtype == RTEN_HIP_DT_F32 ? launch_select<K32<RTEN_HIP_DT_F32>>(ctx, p, x, y) : launch_select<K32<RTEN_HIP_DT_I32>>(ctx, p, x, y);
}

RTEN_EXPORT int32_t rten_hip_arg_minmax_strided(rten_hip_ctx *ctx, int32_t op, int32_t dtype, int32_t n_outer, const int64_t *outer_shape,
                                                const int64_t *outer_strides, int64_t axis_len, int64_t axis_stride, const void *x, int32_t *y) {
    RTEN_CHECK_CTX(ctx);
    SelArgs p;
    if (int32_t rc = select_args(ctx, "arg_minmax", p, op, dtype, n_outer, outer_shape, outer_strides, 1, &axis_len, &axis_stride)) return rc;
    if (axis_len == 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "Cannot select index from empty sequence");
    if (p.rows == 0) return RTEN_HIP_OK;
    if (!x || !y) return RTEN_HIP_ERR_INVALID_VALUE;
    ProfScope ps(ctx, "arg_minmax", 0.0, 4.0 * p.rows * ((double)p.inner + 1));
    return dtype == RTEN_HIP_DT_F32 ? launch_select<K64<RTEN_HIP_DT_F32>>(ctx, p, x, y) : launch_select<K64<RTEN_HIP_DT_I32>>(ctx, p, x, y);
}

RTEN_EXPORT int32_t rten_hip_topk_strided(rten_hip_ctx *ctx, int32_t largest, int32_t dtype, int32_t n_outer, const int64_t *outer_shape,
                                          const int64_t *outer_strides, const int64_t *outer_out_strides, int64_t axis_len, int64_t axis_stride, int64_t k,
                                          const void *x, void *values, int32_t *indices, int64_t out_axis_stride) {
    RTEN_CHECK_CTX(ctx);
    if (dtype != RTEN_HIP_DT_F32 && dtype != RTEN_HIP_DT_I32) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "topk: element type must be float32 or int32");
    // (the level count is refused ahead of the checks on the axis and on k, the levels themselves after them: slice_fill below looks at both)
    if (n_outer < 0 || n_outer > 6 || (n_outer && (!outer_shape || !outer_strides || !outer_out_strides)))
        return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "topk: at most 6 kept dims");
    if (axis_len < 0 || axis_len > 0x7fffffff || axis_stride < 0 || out_axis_stride < 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "topk: bad dimension");
    if (k < 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "k must be positive");
    if (k == 0) return RTEN_HIP_OK;
    if (k > axis_len) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "k > dimension size");
    if (k > 4096) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "topk: k > 4096 is not supported by the device path (a full sort of a long lane is a different kernel)");
    TopkArgs p = {};
    if (int32_t rc = slice_fill(ctx, "topk", n_outer, outer_shape, {outer_strides, outer_out_strides}, p.kept, p.lanes)) return rc;
    if (p.lanes == 0) return RTEN_HIP_OK;
    if (!x || !values || !indices) return RTEN_HIP_ERR_INVALID_VALUE;
    p.axis_len = (int)axis_len;
    p.axis_stride = axis_stride;
    p.k = (int)k;
    p.out_axis_stride = out_axis_stride;
    p.vflip = largest ? 0u : 0xffffffffu;
    ProfScope ps(ctx, "topk", 0.0, 4.0 * p.lanes * ((double)axis_len + 2.0 * k));
    auto launch = [&](const unsigned long long *lin, unsigned long long *lout) -> int32_t {
        const int64_t grid = p.lanes * p.units;
        if (grid > 0x7fffffff) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "topk: more than 2^31 - 1 workgroups in one launch");
        const int threads = p.P / 2 < 64 ? 64 : (p.P / 2 > 1024 ? 1024 : p.P / 2);
        const size_t lds = sizeof(unsigned long long) * (size_t)p.P;
        if (dtype == RTEN_HIP_DT_F32)
            hipLaunchKernelGGL(topk_sort_kernel<RTEN_HIP_DT_F32>, dim3((unsigned)grid), dim3(threads), lds, ctx->stream, p, (const unsigned *)x, lin, lout, (unsigned *)values, indices);
        else
            hipLaunchKernelGGL(topk_sort_kernel<RTEN_HIP_DT_I32>, dim3((unsigned)grid), dim3(threads), lds, ctx->stream, p, (const unsigned *)x, lin, lout, (unsigned *)values, indices);
        RTEN_LAUNCH_CHECK(ctx, "topk_sort_kernel");
        return RTEN_HIP_OK;
    };
    if (axis_len <= 8192) { // the lane fits one workgroup's LDS
        p.P = next_pow2(axis_len) < 128 ? 128 : next_pow2(axis_len);
        p.units = 1;
        p.final = 1;
        return launch(nullptr, nullptr);
    }
    // chunks: small enough to spread a lone lane over the machine, at least 2 k so that a merge always halves the list count
    p.P = next_pow2(2 * k) < 1024 ? 1024 : next_pow2(2 * k);
    p.kk = (int)k;
    const int64_t nchunks = (axis_len + p.P - 1) / p.P;
    // the two list buffers (this launch's output, the previous one's) share the scratch allocation
    const size_t first = sizeof(unsigned long long) * (size_t)(p.lanes * nchunks * p.kk);
    const int per_merge = 8192 / p.kk;
    const size_t second = sizeof(unsigned long long) * (size_t)(p.lanes * ((nchunks + per_merge - 1) / per_merge) * p.kk);
    char *buf = (char *)rten_scratch(ctx, first + second);
    if (!buf) return rten_set_error(ctx, RTEN_HIP_ERR_HIP, "topk: no scratch for %zu bytes of candidate lists", first + second);
    unsigned long long *cur = (unsigned long long *)buf, *other = (unsigned long long *)(buf + first);
    p.units = (int)nchunks;
    p.final = 0;
    if (int32_t rc = launch(nullptr, cur)) return rc;
    p.from_lists = 1;
    p.nlists = (int)nchunks;
    while (true) {
        const int64_t total = (int64_t)p.nlists * p.kk;
        p.P = total >= 8192 ? 8192 : (next_pow2(total) < 128 ? 128 : next_pow2(total));
        p.per = p.P / p.kk;
        p.units = (p.nlists + p.per - 1) / p.per;
        p.final = p.units == 1;
        if (int32_t rc = launch(cur, other)) return rc;
        if (p.final) return RTEN_HIP_OK;
        p.nlists = p.units;
        unsigned long long *t = cur;
        cur = other;
        other = t;
    }
}
