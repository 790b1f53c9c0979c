// CumSum, GatherElements, Trilu and Tile of 4-byte elements (src/ops/reduce.rs:217-297, gather.rs:196-319, trilu.rs:15-64, concat.rs:239-300).
//
// CumSum on the [outer][axis_len][inner] view, per lane along the axis: acc = 0; for x in walking order: prev = acc; acc += x; y = exclusive ? prev : acc.
// The f32 sum is strictly sequential -- each partial sum ONE rounded add, the first `+0.0 + x0` (a leading -0.0 gives +0.0); int32 wraps.  So a lane is
// serial by contract, and the parallelism is across lanes.  Two forms, chosen on the host:
//   * column form (inner > 1): a thread owns one (outer, inner) lane and walks the axis with the running sum in a register, SCAN_AHEAD loads ahead of
//     the adds.  Consecutive threads take consecutive `inner`, so every load and store of a wave is contiguous.  A grid-stride loop covers lane counts
//     past SCAN_MAX_BLOCKS * SCAN_THREADS.
//   * row form (inner == 1): lanes are contiguous rows, and a thread per row would read with a stride of the row length.  A workgroup owns SCAN_ROWS rows
//     and moves along the axis in chunks of SCAN_CHUNK: the [SCAN_ROWS][SCAN_CHUNK] tile is loaded into LDS with consecutive threads on consecutive columns
//     (256 B per wave and row), the first SCAN_ROWS threads each scan their own row's chunk (LDS -> registers -> LDS) carrying the sum from chunk to chunk, and
//     the tile is stored the way it was loaded.  The LDS row pitch is SCAN_CHUNK + 1 dwords: the threads of the scanning wave walk different rows at the same
//     column, and the odd pitch puts the 32 lanes of a half-wave on 32 different banks.  `reverse` walks the chunks, and each chunk, from the end.  The
//     ragged last chunk and row block are masked on load and on store.
// GatherElements, Trilu and Tile are one thread per output element with a grid-stride loop; flat indices are decoded with the exact multiply-shift divider
// of internal.h while the output has fewer than 2^31 elements, with 64-bit division above.
#include "internal.h"

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ROWS = 64;             // row form: rows per workgroup (one wave scans, all four move the tile)
constexpr int SCAN_CHUNK = 64;            // row form: columns per LDS tile
constexpr int SCAN_PITCH = SCAN_CHUNK + 1; // LDS row pitch in dwords
constexpr int SCAN_AHEAD = 16;             // column form: elements of a lane loaded before they are added
constexpr int64_t SCAN_MAX_BLOCKS = 2048; // grid cap of every kernel here (8 workgroups of 256 threads per CU); the loops stride past it

// the wrapping int32 add is done on uint32_t (signed overflow is undefined in C++)
template <typename T> struct ScanAcc;
template <> struct ScanAcc<float> { typedef float type; };
template <> struct ScanAcc<int32_t> { typedef uint32_t type; };

template <typename T>
__global__ __launch_bounds__(SCAN_THREADS) void cumsum_column_kernel(int exclusive, int reverse, int64_t lanes, int64_t axis_len, int64_t inner, const T *__restrict__ x,
                                                                      T *__restrict__ y) {
    typedef typename ScanAcc<T>::type A;
    const int64_t step = (int64_t)gridDim.x * SCAN_THREADS;
    for (int64_t lane = (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x; lane < lanes; lane += step) {
        const int64_t o = lane / inner, i = lane - o * inner;
        const int64_t base = o * axis_len * inner + i;
        A acc = 0;
        int64_t t = 0;
        // SCAN_AHEAD elements are loaded before the first of them is added: the loads do not depend on the running sum, only the adds do, so a lane keeps
        // SCAN_AHEAD loads in flight instead of paying one memory latency per element.  The adds stay in walking order.
        for (; t + SCAN_AHEAD <= axis_len; t += SCAN_AHEAD) {
            A v[SCAN_AHEAD];
#pragma unroll
            for (int u = 0; u < SCAN_AHEAD; u++) v[u] = (A)x[base + (reverse ? axis_len - 1 - (t + u) : t + u) * inner];
#pragma unroll
            for (int u = 0; u < SCAN_AHEAD; u++) {
                const A prev = acc;
                acc = acc + v[u];
                y[base + (reverse ? axis_len - 1 - (t + u) : t + u) * inner] = (T)(exclusive ? prev : acc);
            }
        }
        for (; t < axis_len; t++) {
            const int64_t at = base + (reverse ? axis_len - 1 - t : t) * inner;
            const A prev = acc;
            acc = acc + (A)x[at];
            y[at] = (T)(exclusive ? prev : acc);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(SCAN_THREADS) void cumsum_row_kernel(int exclusive, int reverse, int64_t rows, int64_t axis_len, const T *__restrict__ x, T *__restrict__ y) {
    typedef typename ScanAcc<T>::type A;
    __shared__ A tile[SCAN_ROWS * SCAN_PITCH];
    const int64_t row_blocks = (rows + SCAN_ROWS - 1) / SCAN_ROWS, chunks = (axis_len + SCAN_CHUNK - 1) / SCAN_CHUNK;
    const int col = threadIdx.x % SCAN_CHUNK, row0 = threadIdx.x / SCAN_CHUNK; // tile movement: thread -> (row0 + k * ROWS_PER_PASS, col)
    constexpr int ROWS_PER_PASS = SCAN_THREADS / SCAN_CHUNK;
    for (int64_t rb = blockIdx.x; rb < row_blocks; rb += gridDim.x) {
        const int64_t first_row = rb * SCAN_ROWS;
        const int n_rows = (int)(rows - first_row < SCAN_ROWS ? rows - first_row : SCAN_ROWS);
        A acc = 0; // of row first_row + threadIdx.x (threads below n_rows)
        for (int64_t cw = 0; cw < chunks; cw++) {
            const int64_t c0 = (reverse ? chunks - 1 - cw : cw) * SCAN_CHUNK;
            const int n_cols = (int)(axis_len - c0 < SCAN_CHUNK ? axis_len - c0 : SCAN_CHUNK);
            if (col < n_cols)
                for (int r = row0; r < n_rows; r += ROWS_PER_PASS) tile[r * SCAN_PITCH + col] = (A)x[(first_row + r) * axis_len + c0 + col];
            __syncthreads();
            if ((int)threadIdx.x < n_rows) {
                // the row's chunk goes to registers first (independent LDS reads), is scanned there in walking order, and goes back: the only dependent chain
                // is the adds.  Columns at and past n_cols of a ragged chunk hold stale LDS words: read, never added, never stored to y.
                A *mine = tile + threadIdx.x * SCAN_PITCH;
                A v[SCAN_CHUNK];
#pragma unroll
                for (int j = 0; j < SCAN_CHUNK; j++) v[j] = mine[j];
                if (!reverse) {
#pragma unroll
                    for (int j = 0; j < SCAN_CHUNK; j++)
                        if (j < n_cols) { const A prev = acc; acc = acc + v[j]; v[j] = exclusive ? prev : acc; }
                } else {
#pragma unroll
                    for (int j = SCAN_CHUNK - 1; j >= 0; j--)
                        if (j < n_cols) { const A prev = acc; acc = acc + v[j]; v[j] = exclusive ? prev : acc; }
                }
#pragma unroll
                for (int j = 0; j < SCAN_CHUNK; j++) mine[j] = v[j];
            }
            __syncthreads();
            if (col < n_cols)
                for (int r = row0; r < n_rows; r += ROWS_PER_PASS) y[(first_row + r) * axis_len + c0 + col] = (T)tile[r * SCAN_PITCH + col];
            __syncthreads(); // the next chunk's loads overwrite the tile
        }
    }
}

// ---- flat index -> coordinates over up to 6 axes, innermost first
struct IndexArgs {
    int32_t ndim, axis;
    int64_t n;          // output elements
    int64_t out[6];     // output extent per axis
    int64_t len[6];     // Tile: the operand's extent per axis; GatherElements: unused
    int64_t stride[6];  // the operand's stride per axis, in elements
    int64_t axis_len;   // GatherElements: the operand's extent along `axis`
    RtenDiv out_div[6], len_div[6];
};

// FAST: n < 2^31, every quotient through the multiply-shift divider
template <bool FAST>
__device__ __forceinline__ void split_index(int64_t &r, int64_t extent, const RtenDiv &dv, int64_t &coord) {
    if (FAST) {
        const int q = rten_div((int)r, dv);
        coord = r - (int64_t)q * extent;
        r = q;
    } else {
        const int64_t q = r / extent;
        coord = r - q * extent;
        r = q;
    }
}

template <bool FAST>
__global__ __launch_bounds__(SCAN_THREADS) void gather_elements_kernel(const IndexArgs a, const uint32_t *__restrict__ x, const int32_t *__restrict__ ids, uint32_t *__restrict__ y) {
    const int64_t step = (int64_t)gridDim.x * SCAN_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x; i < a.n; i += step) {
        // normalised and clamped before the address is formed: whatever the index, the read is inside x
        int64_t id = ids[i];
        if (id < 0) id += a.axis_len;
        id = id < 0 ? 0 : (id > a.axis_len - 1 ? a.axis_len - 1 : id);
        int64_t r = i, off = 0;
        for (int d = a.ndim - 1; d >= 0; d--) {
            int64_t c;
            split_index<FAST>(r, a.out[d], a.out_div[d], c);
            off += (d == a.axis ? id : c) * a.stride[d];
        }
        y[i] = x[off];
    }
}

template <bool FAST>
__global__ __launch_bounds__(SCAN_THREADS) void trilu_kernel(int upper, int64_t k, int64_t n, int64_t rows, int64_t cols, RtenDiv rows_div, RtenDiv cols_div,
                                                             const uint32_t *__restrict__ x, uint32_t *__restrict__ y) {
    const int64_t step = (int64_t)gridDim.x * SCAN_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x; i < n; i += step) {
        int64_t r = i, col, row;
        split_index<FAST>(r, cols, cols_div, col);
        split_index<FAST>(r, rows, rows_div, row);
        const int64_t delta = row + k - col;
        const bool keep = upper ? delta <= 0 : delta >= 0;
        const uint32_t v = x[i];
        y[i] = keep ? v : 0u; // a masked element's bits never reach the output
    }
}

template <bool FAST>
__global__ __launch_bounds__(SCAN_THREADS) void tile_kernel(const IndexArgs a, const uint32_t *__restrict__ x, uint32_t *__restrict__ y) {
    const int64_t step = (int64_t)gridDim.x * SCAN_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x; i < a.n; i += step) {
        int64_t r = i, off = 0;
        for (int d = a.ndim - 1; d >= 0; d--) {
            int64_t c, q = 0, s;
            split_index<FAST>(r, a.out[d], a.out_div[d], c);
            q = c;
            split_index<FAST>(q, a.len[d], a.len_div[d], s); // s = c mod len
            off += s * a.stride[d];
        }
        y[i] = x[off];
    }
}

unsigned blocks_for(int64_t n) {
    const int64_t b = ceil_div64(n, SCAN_THREADS);
    return (unsigned)(b < SCAN_MAX_BLOCKS ? b : SCAN_MAX_BLOCKS);
}

constexpr int64_t kLim = 0x7fffffff;

} // namespace

RTEN_EXPORT int32_t rten_hip_cumsum_b32(rten_hip_ctx *ctx, int32_t dtype, int32_t exclusive, int32_t reverse, int64_t outer, int64_t axis_len, int64_t inner, const void *x,
                                        void *y) {
    RTEN_CHECK_CTX(ctx);
    if (dtype != RTEN_HIP_DTYPE_F32 && dtype != RTEN_HIP_DTYPE_I32) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "cumsum: float32 or int32 only");
    if (outer < 0 || axis_len < 0 || inner < 0 || outer > kLim || axis_len > kLim || inner > kLim) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "cumsum: bad dimension");
    if (outer == 0 || axis_len == 0 || inner == 0) return RTEN_HIP_OK;
    if ((double)outer * (double)axis_len * (double)inner >= 9.0e18) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "cumsum: bad dimension");
    if (!x || !y) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "cumsum: null input or output");
    const int ex = exclusive != 0, rev = reverse != 0;
    const bool f32 = dtype == RTEN_HIP_DTYPE_F32;
    ProfScope ps(ctx, inner == 1 ? "cumsum_row_b32" : "cumsum_column_b32", (double)outer * axis_len * inner, 8.0 * outer * axis_len * inner);
    if (inner == 1) {
        const int64_t rb = ceil_div64(outer, SCAN_ROWS);
        const dim3 grid((unsigned)(rb < SCAN_MAX_BLOCKS ? rb : SCAN_MAX_BLOCKS));
        if (f32) hipLaunchKernelGGL(cumsum_row_kernel<float>, grid, dim3(SCAN_THREADS), 0, ctx->stream, ex, rev, outer, axis_len, (const float *)x, (float *)y);
        else hipLaunchKernelGGL(cumsum_row_kernel<int32_t>, grid, dim3(SCAN_THREADS), 0, ctx->stream, ex, rev, outer, axis_len, (const int32_t *)x, (int32_t *)y);
    } else {
        const int64_t lanes = outer * inner;
        const dim3 grid(blocks_for(lanes));
        if (f32) hipLaunchKernelGGL(cumsum_column_kernel<float>, grid, dim3(SCAN_THREADS), 0, ctx->stream, ex, rev, lanes, axis_len, inner, (const float *)x, (float *)y);
        else hipLaunchKernelGGL(cumsum_column_kernel<int32_t>, grid, dim3(SCAN_THREADS), 0, ctx->stream, ex, rev, lanes, axis_len, inner, (const int32_t *)x, (int32_t *)y);
    }
    RTEN_LAUNCH_CHECK(ctx, "cumsum_b32");
    return RTEN_HIP_OK;
}

RTEN_EXPORT int32_t rten_hip_gather_elements_b32(rten_hip_ctx *ctx, int32_t ndim, const int64_t *x_shape, const int64_t *idx_shape, int32_t axis, const void *x,
                                                 const int32_t *ids, void *y) {
    RTEN_CHECK_CTX(ctx);
    if (ndim < 1 || ndim > 6 || !x_shape || !idx_shape || axis < 0 || axis >= ndim) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "gather_elements: 1 to 6 dims, axis inside them");
    IndexArgs a = {};
    a.ndim = ndim; a.axis = axis; a.n = 1;
    double x_words = 1, y_words = 1;
    for (int d = 0; d < ndim; d++) {
        if (x_shape[d] < 0 || idx_shape[d] < 0 || x_shape[d] > kLim || idx_shape[d] > kLim) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "gather_elements: bad dimension");
        if (d != axis && idx_shape[d] > x_shape[d]) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "`indices` size must be <= input size in non-axis dimensions");
        x_words *= (double)x_shape[d];
        y_words *= (double)idx_shape[d];
    }
    if (x_words >= 9.0e18 || y_words >= 9.0e18) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "gather_elements: bad dimension");
    for (int d = 0; d < ndim; d++) a.n *= idx_shape[d];
    if (a.n == 0) return RTEN_HIP_OK;
    if (x_shape[axis] == 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "Entry in `indices` is out of range"); // (nothing to clamp to)
    if (!x || !ids || !y) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "gather_elements: null input, indices or output");
    a.axis_len = x_shape[axis];
    const bool fast = a.n < kLim;
    int64_t acc = 1;
    for (int d = ndim - 1; d >= 0; d--) {
        a.out[d] = idx_shape[d];
        a.stride[d] = acc;
        acc *= x_shape[d];
        if (fast) a.out_div[d] = rten_make_div(a.n, a.out[d]);
    }
    ProfScope ps(ctx, "gather_elements_b32", 0.0, 12.0 * a.n);
    if (fast) hipLaunchKernelGGL(gather_elements_kernel<true>, dim3(blocks_for(a.n)), dim3(SCAN_THREADS), 0, ctx->stream, a, (const uint32_t *)x, ids, (uint32_t *)y);
    else hipLaunchKernelGGL(gather_elements_kernel<false>, dim3(blocks_for(a.n)), dim3(SCAN_THREADS), 0, ctx->stream, a, (const uint32_t *)x, ids, (uint32_t *)y);
    RTEN_LAUNCH_CHECK(ctx, "gather_elements_b32");
    return RTEN_HIP_OK;
}

RTEN_EXPORT int32_t rten_hip_trilu_b32(rten_hip_ctx *ctx, int32_t upper, int64_t k, int64_t batch, int64_t rows, int64_t cols, const void *x, void *y) {
    RTEN_CHECK_CTX(ctx);
    if (batch < 0 || rows < 0 || cols < 0 || batch > kLim || rows > kLim || cols > kLim) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "trilu: bad dimension");
    if (batch == 0 || rows == 0 || cols == 0) return RTEN_HIP_OK;
    if (!x || !y) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "trilu: null input or output");
    if ((double)batch * (double)rows * (double)cols >= 9.0e18) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "trilu: bad dimension");
    const int64_t n = batch * rows * cols;
    const bool fast = n < kLim;
    // |row + k - col| stays far inside 64 bits: row, col < 2^31 and k is brought into [-2^32, 2^32], beyond which every k decides alike
    const int64_t kc = k > ((int64_t)1 << 32) ? ((int64_t)1 << 32) : (k < -((int64_t)1 << 32) ? -((int64_t)1 << 32) : k);
    ProfScope ps(ctx, "trilu_b32", 0.0, 8.0 * n);
    if (fast)
        hipLaunchKernelGGL(trilu_kernel<true>, dim3(blocks_for(n)), dim3(SCAN_THREADS), 0, ctx->stream, upper != 0, kc, n, rows, cols, rten_make_div(n, rows), rten_make_div(n, cols),
                           (const uint32_t *)x, (uint32_t *)y);
    else
        hipLaunchKernelGGL(trilu_kernel<false>, dim3(blocks_for(n)), dim3(SCAN_THREADS), 0, ctx->stream, upper != 0, kc, n, rows, cols, RtenDiv{}, RtenDiv{}, (const uint32_t *)x,
                           (uint32_t *)y);
    RTEN_LAUNCH_CHECK(ctx, "trilu_b32");
    return RTEN_HIP_OK;
}

RTEN_EXPORT int32_t rten_hip_tile_b32(rten_hip_ctx *ctx, int32_t ndim, const int64_t *x_shape, const int64_t *repeats, const void *x, void *y) {
    RTEN_CHECK_CTX(ctx);
    if (ndim < 0 || ndim > 6 || (ndim && (!x_shape || !repeats))) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "tile: more than 6 dims");
    IndexArgs a = {};
    a.ndim = ndim; a.n = 1;
    for (int d = 0; d < ndim; d++) {
        if (repeats[d] < 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "invalid repeats");
        if (x_shape[d] < 0 || x_shape[d] > kLim || repeats[d] > kLim || x_shape[d] * repeats[d] > kLim) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "tile: bad dimension");
        a.out[d] = x_shape[d] * repeats[d];
        a.len[d] = x_shape[d];
        if ((double)a.n * (double)a.out[d] >= 9.0e18) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "tile: bad dimension");
        a.n *= a.out[d];
    }
    if (a.n == 0) return RTEN_HIP_OK;
    if (!x || !y) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "tile: null input or output");
    const bool fast = a.n < kLim;
    int64_t acc = 1;
    for (int d = ndim - 1; d >= 0; d--) {
        a.stride[d] = acc;
        acc *= x_shape[d];
        if (fast) { a.out_div[d] = rten_make_div(a.n, a.out[d]); a.len_div[d] = rten_make_div(a.out[d], a.len[d]); }
    }
    ProfScope ps(ctx, "tile_b32", 0.0, 8.0 * a.n);
    if (fast) hipLaunchKernelGGL(tile_kernel<true>, dim3(blocks_for(a.n)), dim3(SCAN_THREADS), 0, ctx->stream, a, (const uint32_t *)x, (uint32_t *)y);
    else hipLaunchKernelGGL(tile_kernel<false>, dim3(blocks_for(a.n)), dim3(SCAN_THREADS), 0, ctx->stream, a, (const uint32_t *)x, (uint32_t *)y);
    RTEN_LAUNCH_CHECK(ctx, "tile_b32");
    return RTEN_HIP_OK;
}
