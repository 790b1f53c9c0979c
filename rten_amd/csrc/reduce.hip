// The Reduce* family on strided views and LpNormalization.
// Replaces src/ops/reduce.rs:414-520 (the outer loop), :523-541 ReduceMean, :590-604 ReduceL2, :653-667 ReduceLogSum, :710-732 ReduceLogSumExp,
// :775-804 ReduceL1, :1046-1059 ReduceProd, :1101-1124 ReduceSum, :1167-1192 ReduceSumSquare, rten-vecmath/src/sum.rs:12-159 and
// src/ops/norm.rs:611-650,705-755 (lp_normalization).
//
// Output element r (row-major over the kept dims) is the kernel's value for the slice spanned by the reduced dims walked in row-major order -- the order in
// which the reference packs a non-contiguous slice (reduce.rs:470-505).  The view is read in place through its strides: nothing is packed.
//
//   Sum, SumAbs, SumSquare   fold_unroll<4> over 16-lane vectors (rten-simd/src/iter.rs:97-120): a 64-lane wavefront IS the four unrolled accumulators side by
//                            side (rowreduce.h); four kernel forms, each parameterised by the element map and the finish (none / sqrt / ln)
//   SumExpSub                a plain fold with ONE 16-lane accumulator (sum.rs:144-158): element i goes into lane i % 16, in order
//   Prod                     one sequential multiply chain per slice (Iterator::product): the parallelism is across slices
//   int32 L1 / SumSquare / Prod   wrapping arithmetic, which is associative and commutative: any order
// No kernel waits for another workgroup, uses scratch memory or reports to the host: every launch can be captured.
#include <cmath>

#include "internal.h"
#include "rowreduce.h" // lane_bcast, simd16_reduce: the reduction order
#include "slice.h"     // the kept / reduced levels and their addressing
#include "vecmath.h"

namespace {

constexpr int ROWS_PER_BLOCK = 4;

struct ReduceArgs {
    SliceLevels<1> kept, red;
    int64_t rows;
    int inner;
    float divisor; // 0: the plain value; slice length: ReduceMean = Sum / len (reduce.rs:532-537)
};

// ------------------------------------------------------------------------------------------------
// Sum / SumAbs / SumSquare in the fold_unroll<4> order.  MAP is simd16_reduce's KIND (the fold of one element into its accumulator); the accumulators are
// merged, and the 16 lane totals added, by plain adds whatever the map (sum.rs:27-33,60-66,86-92).  FIN is what the operator does to the total.
// ------------------------------------------------------------------------------------------------
constexpr int MAP_ID = 0, MAP_SQUARE = 1, MAP_ABS = 2;
constexpr int FIN_NONE = 0, FIN_SQRT = 1, FIN_LN = 2;

template <int MAP>
__device__ __forceinline__ float fold_elem(float acc, float x) {
    if constexpr (MAP == MAP_ID) return acc + x;
    else if constexpr (MAP == MAP_SQUARE) return vm::fma(x, x, acc);
    else return acc + __builtin_fabsf(x);
}

// ln: the f64 logarithm of the total rounded to f32 once (the reference calls the host's libm; docs/KERNELS.md 4.7, 4.8)
template <int FIN>
__device__ __forceinline__ float finish_total(float s, float divisor) {
    if constexpr (FIN == FIN_SQRT) return __builtin_sqrtf(s);
    else if constexpr (FIN == FIN_LN) return (float)log((double)s);
    else return divisor != 0.f ? s / divisor : s;
}

template <int MAP, int FIN>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void reduce_sum_kernel(const ReduceArgs p, const float *__restrict__ x, float *__restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const float *xr = x + slice_row_base(p.kept, p.rows, row);
    auto get = [&](int i) -> float { return xr[slice_elem_off(p.red, i)]; };
    const float s = simd16_reduce<MAP>(get, p.inner, 0.f, lane);
    if (lane == 0) y[row] = finish_total<FIN>(s, p.divisor);
}

// Slices of at most 16 * EPL elements: four output elements per wave, one per 16-lane DPP row (global_avg_pool_rows16_kernel's
// scheme).  Lane l owns elements l + 16 q -- the ones the reference's accumulator lane l adds: the first 4 * (n / 64) of them
// go round-robin into the four unrolled accumulators, which fold left to right; the rest (whole vectors, masked tail) are
// added to the folded value one by one (rten-simd/src/iter.rs:97-120).
template <int EPL, int MAP, int FIN>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void reduce_sum_rows16_kernel(const ReduceArgs p, const float *__restrict__ x, float *__restrict__ y) {
    const int lane = threadIdx.x & 63, l = lane & 15;
    const int64_t row = ((int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    const int64_t rr = row < p.rows ? row : p.rows - 1;
    const float *xr = x + slice_row_base(p.kept, p.rows, rr);
    float v[EPL];
#pragma unroll
    for (int q = 0; q < EPL; q++) v[q] = xr[slice_elem_off(p.red, l + 16 * q < p.inner ? l + 16 * q : 0)];
    const int unrolled = (p.inner >> 6) * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < EPL; q++)
        if (q < unrolled) acc[q & 3] = fold_elem<MAP>(acc[q & 3], v[q]);
    float a = ((acc[0] + acc[1]) + acc[2]) + acc[3];
#pragma unroll
    for (int q = 0; q < EPL; q++)
        if (q >= unrolled && l + 16 * q < p.inner) a = fold_elem<MAP>(a, v[q]);
    float s = a;
#pragma unroll
    for (int k = 1; k < 16; k++) s = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x111, 0xf, 0xf, true)) + a;
    if (l == 15 && row < p.rows) y[row] = finish_total<FIN>(s, p.divisor);
}

// Reduced axes strided, innermost kept axis contiguous (a column sum): a wave-per-row walk would touch 64 cache lines per
// load.  Here a 1024-thread workgroup owns 16 adjacent output elements j; wave w is the reference's accumulator lane l = w and
// its lanes are (u = unrolled accumulator, j): every load instruction reads four 64-byte runs.  Each thread's chain is the
// reference's acc[u][l]; the fold over u is three lane shuffles, the in-order sum over l goes through LDS.
template <int MAP, int FIN>
__global__ __launch_bounds__(1024) void reduce_sum_cols_kernel(const ReduceArgs p, const float *__restrict__ x, float *__restrict__ y) {
    __shared__ float part[16][16];
    const int lane = threadIdx.x & 63, l = threadIdx.x >> 6, u = lane >> 4, j = lane & 15;
    const int last = p.kept.shape[p.kept.n - 1];
    const int groups = (last + 15) >> 4;
    // Two neighbouring column groups read the two 64-byte halves of the same 128-byte lines.  Workgroup ids go round-robin over the eight XCDs, so
    // neighbours in id order never share an L2 and every line is fetched twice; here each XCD gets a CONTIGUOUS run of groups (ids id, id + 8, ...
    // are dispatched to the same XCD one after the other), and the second half of a line is an L2 hit.
    unsigned bid = blockIdx.x;
    {
        const unsigned nt = gridDim.x, xcd = bid & 7, qn = nt >> 3, rn = nt & 7;
        bid = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + (bid >> 3);
    }
    const int64_t prefix = bid / groups;
    const int j0 = (int)(bid - prefix * groups) * 16;
    const int jj = j0 + j < last ? j0 + j : last - 1;
    const int64_t row = prefix * last + jj;
    const float *xr = x + slice_row_base(p.kept, p.rows, row);
    const int n = p.inner, full4 = n >> 6;
    // The chain of adds is the reference's (one accumulator, elements in order); the LOADS are independent, so eight are requested before the
    // first add -- a load per add made this kernel one memory round trip per element (31.5 us for 4096 x 3072 -> 3072: round 3).
    float acc = 0.f;
    int c = 0;
    for (; c + 16 <= full4; c += 16) {
        float tv[16];
#pragma unroll
        for (int k = 0; k < 16; k++) tv[k] = xr[slice_elem_off(p.red, (c + k) * 64 + u * 16 + l)];
#pragma unroll
        for (int k = 0; k < 16; k++) acc = fold_elem<MAP>(acc, tv[k]);
    }
    for (; c + 8 <= full4; c += 8) {
        float tv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) tv[k] = xr[slice_elem_off(p.red, (c + k) * 64 + u * 16 + l)];
#pragma unroll
        for (int k = 0; k < 8; k++) acc = fold_elem<MAP>(acc, tv[k]);
    }
    for (; c < full4; c++) acc = fold_elem<MAP>(acc, xr[slice_elem_off(p.red, c * 64 + u * 16 + l)]);
    float a = lane_bcast(acc, j);
    a = a + lane_bcast(acc, j + 16);
    a = a + lane_bcast(acc, j + 32);
    a = a + lane_bcast(acc, j + 48);
    int i0 = full4 * 64;
    for (; i0 + 16 <= n; i0 += 16) a = fold_elem<MAP>(a, xr[slice_elem_off(p.red, i0 + l)]);
    if (i0 + l < n) a = fold_elem<MAP>(a, xr[slice_elem_off(p.red, i0 + l)]);
    if (u == 0) part[l][j] = a;
    __syncthreads();
    if (threadIdx.x < 16 && j0 + (int)threadIdx.x < last) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; k++) s = s + part[k][threadIdx.x];
        y[prefix * last + j0 + threadIdx.x] = finish_total<FIN>(s, p.divisor);
    }
}

// The reduced axes are strided and the innermost kept axis is contiguous, with enough of it for 16 adjacent outputs: the column forms' condition.
bool column_layout(const ReduceArgs &p) {
    const int64_t last = p.kept.n ? p.kept.shape[p.kept.n - 1] : 1;
    return p.inner > 64 && p.kept.n && p.kept.stride[0][p.kept.n - 1] == 1 && last >= 16 && p.red.stride[0][p.red.n - 1] > 1;
}

template <int MAP, int FIN>
void launch_sum(rten_hip_ctx *ctx, const ReduceArgs &p, const float *x, float *y) {
    const dim3 block(64 * ROWS_PER_BLOCK);
    const dim3 grid16((unsigned)((p.rows + 4 * ROWS_PER_BLOCK - 1) / (4 * ROWS_PER_BLOCK)));
    const int64_t last = p.kept.n ? p.kept.shape[p.kept.n - 1] : 1;
    if (column_layout(p))
        hipLaunchKernelGGL((reduce_sum_cols_kernel<MAP, FIN>), dim3((unsigned)(p.rows / last * ((last + 15) / 16))), dim3(1024), 0, ctx->stream, p, x, y);
    else if (p.inner <= 64) hipLaunchKernelGGL((reduce_sum_rows16_kernel<4, MAP, FIN>), grid16, block, 0, ctx->stream, p, x, y);
    else if (p.inner <= 128) hipLaunchKernelGGL((reduce_sum_rows16_kernel<8, MAP, FIN>), grid16, block, 0, ctx->stream, p, x, y);
    else if (p.inner <= 256) hipLaunchKernelGGL((reduce_sum_rows16_kernel<16, MAP, FIN>), grid16, block, 0, ctx->stream, p, x, y);
    else
        hipLaunchKernelGGL((reduce_sum_kernel<MAP, FIN>), dim3((unsigned)((p.rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), block, 0, ctx->stream, p, x, y);
}

// ------------------------------------------------------------------------------------------------
// ReduceLogSumExp (reduce.rs:710-732): m = MaxNum(slice) (a NaN anywhere gives NaN); a non-finite m is the result; otherwise m + ln(SumExpSub(slice, m)).
// SumExpSub (sum.rs:144-158) is a plain fold: ONE 16-lane accumulator, element i added into lane i % 16 in order, exp = the full-range Exp; the 16 lanes
// are then added from lane 0.  One wave per slice, one launch: the slice stays in registers up to 64 * CH elements (LogSoftmax's register form);
// CH == 0 reads it twice.
// ------------------------------------------------------------------------------------------------
template <int CH>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void reduce_lse_kernel(const ReduceArgs p, const float *__restrict__ x, float *__restrict__ y) {
    const int lane = threadIdx.x & 63, l = lane & 15;
    const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const float *xr = x + slice_row_base(p.kept, p.rows, row);
    const int n = p.inner;
    [[maybe_unused]] float v[CH > 0 ? CH : 1];
    float mx = -__builtin_inff();
    bool nan = false;
    if constexpr (CH > 0) {
#pragma unroll
        for (int k = 0; k < CH; k++) {
            const int i = k * 64 + lane;
            v[k] = xr[slice_elem_off(p.red, i < n ? i : 0)];
        }
#pragma unroll
        for (int k = 0; k < CH; k++)
            if (k * 64 + lane < n) { nan = nan || v[k] != v[k]; mx = fmaxf(mx, v[k]); }
    } else {
        for (int i = lane; i < n; i += 64) {
            const float t = xr[slice_elem_off(p.red, i)];
            nan = nan || t != t;
            mx = fmaxf(mx, t);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float m = __any(nan) ? __builtin_nanf("") : mx;
    // (a non-finite m: the sum below is computed and dropped -- x - m is then NaN or -inf for every element, which faults nothing)
    float a = 0.f;
    auto add_chunk = [&](int k, float e) { // the four 16-lane vectors of chunk k, in order, into the one accumulator
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float eq = lane_bcast(e, l + 16 * q);
            if (k * 64 + l + 16 * q < n) a = a + eq;
        }
    };
    if constexpr (CH > 0) {
#pragma unroll
        for (int k = 0; k < CH; k++)
            if (k * 64 < n) add_chunk(k, vm::exp_full(v[k] - m));
    } else {
        const int nch = (n + 63) / 64;
        for (int k = 0; k < nch; k++) {
            const int i = k * 64 + lane;
            add_chunk(k, vm::exp_full(xr[slice_elem_off(p.red, i < n ? i : 0)] - m));
        }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k++) s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), k));
    const bool finite = (__float_as_uint(m) & 0x7f800000u) != 0x7f800000u;
    if (lane == 0) y[row] = finite ? m + (float)log((double)s) : m;
}

// ------------------------------------------------------------------------------------------------
// ReduceProd, f32 (reduce.rs:1046-1059): ((1 * s0) * s1) * ... -- float multiplication is not associative, so each slice is ONE chain in element order and
// a thread owns a slice.  The loads do not depend on the chain: they are requested in batches ahead of it.
// ------------------------------------------------------------------------------------------------
constexpr int PROD_BATCH = 16;

// column layout: adjacent threads own adjacent outputs, whose elements are adjacent in memory -- every load instruction reads one 256-byte run
__global__ __launch_bounds__(64) void reduce_prod_cols_kernel(const ReduceArgs p, const float *__restrict__ x, float *__restrict__ y) {
    const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= p.rows) return;
    const float *xr = x + slice_row_base(p.kept, p.rows, row);
    const int n = p.inner;
    float acc = 1.0f;
    int i = 0;
    for (; i + PROD_BATCH <= n; i += PROD_BATCH) {
        float tv[PROD_BATCH];
#pragma unroll
        for (int k = 0; k < PROD_BATCH; k++) tv[k] = xr[slice_elem_off(p.red, i + k)];
#pragma unroll
        for (int k = 0; k < PROD_BATCH; k++) acc = acc * tv[k];
    }
    for (; i < n; i++) acc = acc * xr[slice_elem_off(p.red, i)];
    y[row] = acc;
}

// any other layout: a wave owns 64 slices and brings them in 64-element pieces through LDS -- lane t LOADS element (piece + t) of each of the 64 slices in
// turn (one run of consecutive elements per instruction when the reduced axis is contiguous, 64 loads in flight), then MULTIPLIES along slice t.  The
// tile row is 65 floats: both the stores (row k, column t) and the reads (row t, column k) touch 64 different banks.
__global__ __launch_bounds__(64) void reduce_prod_rows_kernel(const ReduceArgs p, const float *__restrict__ x, float *__restrict__ y) {
    __shared__ float tile[64][65];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * 64;
    const int nrows = (int)(p.rows - row0 < 64 ? p.rows - row0 : 64);
    const int n = p.inner;
    float acc = 1.0f;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int64_t eo = slice_elem_off(p.red, i0 + t < n ? i0 + t : 0);
        for (int k0 = 0; k0 < nrows; k0 += 16) {
            float tv[16];
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int r = k0 + k < nrows ? k0 + k : nrows - 1;
                tv[k] = x[slice_row_base(p.kept, p.rows, row0 + r) + eo];
            }
#pragma unroll
            for (int k = 0; k < 16; k++) tile[k0 + k][t] = tv[k];
        }
        __syncthreads();
        const int m = n - i0 < 64 ? n - i0 : 64;
        if (t < nrows) {
            int k = 0;
            for (; k + 16 <= m; k += 16) {
                float tv[16];
#pragma unroll
                for (int q = 0; q < 16; q++) tv[q] = tile[t][k + q];
#pragma unroll
                for (int q = 0; q < 16; q++) acc = acc * tv[q];
            }
            for (; k < m; k++) acc = acc * tile[t][k];
        }
        __syncthreads();
    }
    if (t < nrows) y[row0 + t] = acc;
}

// ------------------------------------------------------------------------------------------------
// int32 ReduceL1 / ReduceSumSquare / ReduceProd (the reference's generic kernels, reduce.rs:782-794,1052-1057,1174-1181): two's complement wrapping
// arithmetic in uint32, so any order gives the same bits.  One wave per slice.
// ------------------------------------------------------------------------------------------------
constexpr int IOP_ABS = 0, IOP_SQUARE = 1, IOP_PROD = 2;

template <int IOP>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void reduce_i32_kernel(const ReduceArgs p, const uint32_t *__restrict__ x, uint32_t *__restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const uint32_t *xr = x + slice_row_base(p.kept, p.rows, row);
    uint32_t acc = IOP == IOP_PROD ? 1u : 0u;
    for (int i = lane; i < p.inner; i += 64) {
        const uint32_t t = xr[slice_elem_off(p.red, i)];
        if constexpr (IOP == IOP_ABS) acc += (t & 0x80000000u) ? 0u - t : t; // `if x < 0 { -x }`: i32::MIN stays (wrapping)
        else if constexpr (IOP == IOP_SQUARE) acc += t * t;
        else acc *= t;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)acc, o, 64);
        acc = IOP == IOP_PROD ? acc * other : acc + other;
    }
    if (lane == 0) y[row] = acc;
}

// ------------------------------------------------------------------------------------------------
// LpNormalization (norm.rs:622-650): norm = SumAbs(lane) (p = 1) or sqrt(SumSquare(lane)) (p = 2) in the fold_unroll<4> order; a zero norm zeroes the
// lane; otherwise y = x * (1 / norm): one IEEE division, one multiply per element.  One wave per lane, lanes read and written through the axis stride;
// the output is contiguous in the input's dim order, so a lane has the same base and stride in x and y.
//   CH > 0: the lane in registers (<= 64 * CH elements): one read, one write.  y may equal x: a wave reads its whole lane before it stores.
//   CH == 0: streaming, any length: the lane is read twice (the second read of a short lane is an L2 hit).  y may equal x: the reduction has finished
//            before the wave's first store, and the second pass reads each element before it stores it.
// ------------------------------------------------------------------------------------------------
struct LpArgs {
    SliceLevels<1> kept;
    int64_t rows;
    int64_t len, stride;
};

template <int CH, int MAP>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void lp_normalize_kernel(const LpArgs p, const float *x, float *y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const int64_t base = slice_row_base(p.kept, p.rows, row);
    const float *xr = x + base;
    float *yr = y + base;
    const int64_t n = p.len, st = p.stride;
    auto get = [&](int64_t i) -> float { return xr[i * st]; };
    float total;
    [[maybe_unused]] float v[CH > 0 ? CH : 1];
    if constexpr (CH > 0) {
#pragma unroll
        for (int k = 0; k < CH; k++) { const int i = k * 64 + lane; v[k] = i < n ? xr[(int64_t)i * st] : 0.f; }
        // simd16_reduce's order, the full chunks from registers (layer_norm_kernel's `red`)
        float acc = 0.f;
        const int full4 = (int)(n / 64);
#pragma unroll
        for (int k = 0; k < CH; k++)
            if (k < full4) acc = fold_elem<MAP>(acc, v[k]);
        float a = acc;
        a = a + lane_bcast(acc, (lane & 15) + 16);
        a = a + lane_bcast(acc, (lane & 15) + 32);
        a = a + lane_bcast(acc, (lane & 15) + 48);
        int i0 = full4 * 64;
        const int l = lane & 15;
        for (; i0 + 16 <= n; i0 += 16) a = fold_elem<MAP>(a, get(i0 + l)); // the < 64-element remainder: cross-lane, served from L1 (before any store of this wave)
        if (i0 + l < n) a = fold_elem<MAP>(a, get(i0 + l));
        total = 0.f;
#pragma unroll
        for (int k = 0; k < 16; k++) total = total + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), k));
    } else {
        total = simd16_reduce<MAP, 8>(get, n, 0.f, lane);
    }
    const float norm = MAP == MAP_SQUARE ? __builtin_sqrtf(total) : total;
    const bool zero = norm == 0.f;
    const float recip = 1.0f / norm;
    if constexpr (CH > 0) {
#pragma unroll
        for (int k = 0; k < CH; k++) {
            const int i = k * 64 + lane;
            if (i < n) yr[(int64_t)i * st] = zero ? 0.f : v[k] * recip;
        }
    } else {
        for (int64_t i = lane; i < n; i += 64) yr[i * st] = zero ? 0.f : xr[i * st] * recip;
    }
}

int32_t reduce_sum_or_mean(rten_hip_ctx *ctx, bool mean, int32_t n_outer, const int64_t *outer_shape, const int64_t *outer_strides, int32_t n_inner,
                           const int64_t *inner_shape, const int64_t *inner_strides, const float *x, float *y) {
    RTEN_CHECK_CTX(ctx);
    ReduceArgs p = {};
    if (int32_t rc = slice_fill(ctx, "reduce_sum", n_outer, outer_shape, {outer_strides}, p.kept, p.rows, n_inner, inner_shape, inner_strides, &p.red, &p.inner)) return rc;
    p.divisor = mean ? (float)p.inner : 0.f;
    if (p.rows == 0) return RTEN_HIP_OK;
    if (!y) return RTEN_HIP_ERR_INVALID_VALUE;
    if (p.inner == 0) { // an empty slice gives the kernel's value for it (reduce.rs:446-452): Sum 0, Mean 0 / 0 = NaN
        RTEN_HIP_TRY(ctx, hipMemsetAsync(y, mean ? 0xff : 0, sizeof(float) * (size_t)p.rows, ctx->stream));
        return RTEN_HIP_OK;
    }
    if (!x) return RTEN_HIP_ERR_INVALID_VALUE;
    ProfScope ps(ctx, "reduce_sum_f32", 0.0, 4.0 * p.rows * ((double)p.inner + 1));
    launch_sum<MAP_ID, FIN_NONE>(ctx, p, x, y);
    RTEN_LAUNCH_CHECK(ctx, "reduce_sum_kernel");
    return RTEN_HIP_OK;
}

} // namespace

RTEN_EXPORT int32_t rten_hip_reduce_sum_strided_f32(rten_hip_ctx *ctx, int32_t n_outer, const int64_t *outer_shape, const int64_t *outer_strides,
                                                    int32_t n_inner, const int64_t *inner_shape, const int64_t *inner_strides,
                                                    const float *x, float *y) {
    return reduce_sum_or_mean(ctx, false, n_outer, outer_shape, outer_strides, n_inner, inner_shape, inner_strides, x, y);
}

RTEN_EXPORT int32_t rten_hip_reduce_mean_strided_f32(rten_hip_ctx *ctx, int32_t n_outer, const int64_t *outer_shape, const int64_t *outer_strides,
                                                     int32_t n_inner, const int64_t *inner_shape, const int64_t *inner_strides,
                                                     const float *x, float *y) {
    return reduce_sum_or_mean(ctx, true, n_outer, outer_shape, outer_strides, n_inner, inner_shape, inner_strides, x, y);
}

RTEN_EXPORT int32_t rten_hip_reduce_strided(rten_hip_ctx *ctx, int32_t kind, int32_t dtype, int32_t n_outer, const int64_t *outer_shape,
                                            const int64_t *outer_strides, int32_t n_inner, const int64_t *inner_shape, const int64_t *inner_strides,
                                            const void *xv, void *yv) {
    RTEN_CHECK_CTX(ctx);
    if (kind < RTEN_HIP_REDUCE_L1 || kind > RTEN_HIP_REDUCE_PROD) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "reduce: unknown kind %d", kind);
    if (dtype != RTEN_HIP_DT_F32 && dtype != RTEN_HIP_DT_I32) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "reduce: unknown element type %d", dtype);
    const bool i32 = dtype == RTEN_HIP_DT_I32;
    if (i32 && (kind == RTEN_HIP_REDUCE_L2 || kind == RTEN_HIP_REDUCE_LOG_SUM || kind == RTEN_HIP_REDUCE_LOG_SUM_EXP))
        return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "reduce: kind %d takes float32 only", kind);
    ReduceArgs p = {};
    if (int32_t rc = slice_fill(ctx, "reduce", n_outer, outer_shape, {outer_strides}, p.kept, p.rows, n_inner, inner_shape, inner_strides, &p.red, &p.inner)) return rc;
    if (p.rows == 0) return RTEN_HIP_OK;
    if (!yv) return RTEN_HIP_ERR_INVALID_VALUE;
    if (p.inner == 0) { // the kernel's value for an empty slice (reduce.rs:446-452): sums 0, Prod 1, LogSum ln(0) = -inf, LogSumExp MaxNum's -inf
        unsigned bits = 0;
        if (kind == RTEN_HIP_REDUCE_PROD) bits = i32 ? 1u : 0x3f800000u;
        else if (kind == RTEN_HIP_REDUCE_LOG_SUM || kind == RTEN_HIP_REDUCE_LOG_SUM_EXP) bits = 0xff800000u;
        RTEN_HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)yv, (int)bits, (size_t)p.rows, ctx->stream));
        return RTEN_HIP_OK;
    }
    if (!xv) return RTEN_HIP_ERR_INVALID_VALUE;
    const dim3 block(64 * ROWS_PER_BLOCK);
    const int64_t wave_blocks = (p.rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    if (wave_blocks > 0x7fffffff) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "reduce: more than 2^33 slices");
    static const char *const names[] = {"reduce_l1", "reduce_sum_square", "reduce_l2", "reduce_log_sum", "reduce_log_sum_exp", "reduce_prod"};
    // (LogSumExp's register form reads once; above it, twice)
    ProfScope ps(ctx, names[kind], 0.0, 4.0 * p.rows * ((kind == RTEN_HIP_REDUCE_LOG_SUM_EXP && p.inner > 1024 ? 2.0 : 1.0) * p.inner + 1));
    if (i32) {
        const uint32_t *x = (const uint32_t *)xv;
        uint32_t *y = (uint32_t *)yv;
        const dim3 grid((unsigned)wave_blocks);
        if (kind == RTEN_HIP_REDUCE_L1) hipLaunchKernelGGL(reduce_i32_kernel<IOP_ABS>, grid, block, 0, ctx->stream, p, x, y);
        else if (kind == RTEN_HIP_REDUCE_SUM_SQUARE) hipLaunchKernelGGL(reduce_i32_kernel<IOP_SQUARE>, grid, block, 0, ctx->stream, p, x, y);
        else hipLaunchKernelGGL(reduce_i32_kernel<IOP_PROD>, grid, block, 0, ctx->stream, p, x, y);
        RTEN_LAUNCH_CHECK(ctx, "reduce_i32_kernel");
        return RTEN_HIP_OK;
    }
    const float *x = (const float *)xv;
    float *y = (float *)yv;
    switch (kind) {
    case RTEN_HIP_REDUCE_L1: launch_sum<MAP_ABS, FIN_NONE>(ctx, p, x, y); break;
    case RTEN_HIP_REDUCE_SUM_SQUARE: launch_sum<MAP_SQUARE, FIN_NONE>(ctx, p, x, y); break;
    case RTEN_HIP_REDUCE_L2: launch_sum<MAP_SQUARE, FIN_SQRT>(ctx, p, x, y); break;
    case RTEN_HIP_REDUCE_LOG_SUM: launch_sum<MAP_ID, FIN_LN>(ctx, p, x, y); break;
    case RTEN_HIP_REDUCE_LOG_SUM_EXP: {
        const dim3 grid((unsigned)wave_blocks);
        if (p.inner <= 256) hipLaunchKernelGGL(reduce_lse_kernel<4>, grid, block, 0, ctx->stream, p, x, y);
        else if (p.inner <= 1024) hipLaunchKernelGGL(reduce_lse_kernel<16>, grid, block, 0, ctx->stream, p, x, y);
        else hipLaunchKernelGGL(reduce_lse_kernel<0>, grid, block, 0, ctx->stream, p, x, y);
        break;
    }
    default: {
        const dim3 grid((unsigned)((p.rows + 63) / 64));
        const bool cols = p.kept.n && p.kept.stride[0][p.kept.n - 1] == 1 && p.kept.shape[p.kept.n - 1] >= 16 && p.red.stride[0][p.red.n - 1] > 1;
        if (cols) hipLaunchKernelGGL(reduce_prod_cols_kernel, grid, dim3(64), 0, ctx->stream, p, x, y);
        else hipLaunchKernelGGL(reduce_prod_rows_kernel, grid, dim3(64), 0, ctx->stream, p, x, y);
        break;
    }
    }
    RTEN_LAUNCH_CHECK(ctx, "reduce_kernel");
    return RTEN_HIP_OK;
}

RTEN_EXPORT int32_t rten_hip_lp_normalize_f32(rten_hip_ctx *ctx, int32_t p_norm, int32_t n_outer, const int64_t *outer_shape, const int64_t *outer_strides,
                                              int64_t axis_len, int64_t axis_stride, const float *x, float *y) {
    RTEN_CHECK_CTX(ctx);
    if (p_norm != 1 && p_norm != 2) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "`p` must be 1 or 2");
    LpArgs p = {};
    if (int32_t rc = slice_fill(ctx, "lp_normalize", n_outer, outer_shape, {outer_strides}, p.kept, p.rows)) return rc;
    if (axis_len < 0 || axis_stride < 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "lp_normalize: bad dimension");
    p.len = axis_len;
    p.stride = axis_stride;
    if (p.rows == 0 || axis_len == 0) return RTEN_HIP_OK; // norm.rs:711-713
    if (!x || !y) return RTEN_HIP_ERR_INVALID_VALUE;
    const int64_t blocks = (p.rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    if (blocks > 0x7fffffff) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "lp_normalize: more than 2^33 lanes");
    const dim3 grid((unsigned)blocks), block(64 * ROWS_PER_BLOCK);
    ProfScope ps(ctx, "lp_normalize_f32", 0.0, (axis_len <= 1024 ? 8.0 : 12.0) * p.rows * axis_len);
#define LP_LAUNCH(CH) do { if (p_norm == 1) hipLaunchKernelGGL((lp_normalize_kernel<CH, MAP_ABS>), grid, block, 0, ctx->stream, p, x, y); \
                           else hipLaunchKernelGGL((lp_normalize_kernel<CH, MAP_SQUARE>), grid, block, 0, ctx->stream, p, x, y); } while (0)
    if (axis_len <= 128) LP_LAUNCH(2);
    else if (axis_len <= 256) LP_LAUNCH(4);
    else if (axis_len <= 512) LP_LAUNCH(8);
    else if (axis_len <= 768) LP_LAUNCH(12);
    else if (axis_len <= 1024) LP_LAUNCH(16);
    else LP_LAUNCH(0);
#undef LP_LAUNCH
    RTEN_LAUNCH_CHECK(ctx, "lp_normalize_kernel");
    return RTEN_HIP_OK;
}
