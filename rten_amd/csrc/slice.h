// The slice description of the strided reductions (reduce.hip, select.hip): a view is split into kept dims, one output element ("row") per
// combination, and reduced dims, the elements of a row's slice in row-major order.  Neighbouring dims are merged by the caller; at most 6 levels of each
// reach the kernels, which turn a row number and an element number back into offsets (in elements) through the view's strides.
#pragma once
#include <hip/hip_runtime.h>

#include "internal.h"

constexpr int SLICE_MAX_LEVELS = 6;

// NS stride lists over one shape list: TopK walks the kept dims of its input and of its outputs together
template <int NS = 1>
struct SliceLevels {
    int n;
    int32_t shape[SLICE_MAX_LEVELS];
    int64_t stride[NS][SLICE_MAX_LEVELS];
};

// Offsets of row `row` of `rows`, one per stride list.  The outermost level needs no division -- what is left of the row index IS its coordinate -- and
// a 64-bit division is ~100 instructions on this machine: with one per row the last-axis kernels were division-bound, 10 us for 49152 rows of 128.
// 32-bit arithmetic whenever the row count allows.
template <int NS>
__host__ __device__ __forceinline__ void slice_row_bases(const SliceLevels<NS> &k, int64_t rows, int64_t row, int64_t (&off)[NS]) {
    for (int s = 0; s < NS; s++) off[s] = 0;
    if (k.n <= 0) return;
    if (rows <= 0x7fffffff) {
        unsigned r = (unsigned)row;
        for (int d = k.n - 1; d > 0; d--) {
            const unsigned q = r / (unsigned)k.shape[d];
            for (int s = 0; s < NS; s++) off[s] += (int64_t)(r - q * (unsigned)k.shape[d]) * k.stride[s][d];
            r = q;
        }
        for (int s = 0; s < NS; s++) off[s] += (int64_t)r * k.stride[s][0];
        return;
    }
    int64_t r = row;
    for (int d = k.n - 1; d > 0; d--) {
        const int64_t q = r / k.shape[d];
        for (int s = 0; s < NS; s++) off[s] += (r - q * k.shape[d]) * k.stride[s][d];
        r = q;
    }
    for (int s = 0; s < NS; s++) off[s] += r * k.stride[s][0];
}
__host__ __device__ __forceinline__ int64_t slice_row_base(const SliceLevels<1> &k, int64_t rows, int64_t row) {
    int64_t off[1];
    slice_row_bases(k, rows, row, off);
    return off[0];
}

// Offset of element i of a slice (fewer than 2^31 elements) from its row base
__host__ __device__ __forceinline__ int64_t slice_elem_off(const SliceLevels<1> &red, int i) {
    if (red.n == 1) return (int64_t)i * red.stride[0][0];
    int r = i;
    int64_t off = 0;
    for (int d = red.n - 1; d >= 0; d--) {
        const int q = r / red.shape[d];
        off += (int64_t)(r - q * red.shape[d]) * red.stride[0][d];
        r = q;
    }
    return off;
}

// The ABI side: checks the pointer lists of a strided entry point and fills the kept levels and the row count and, when `red` is given, the reduced
// levels (always at least one: no reduced dims is one level of one element) and the slice length.  `what` names the entry point in the messages.
template <int NS>
inline int32_t slice_fill(rten_hip_ctx *ctx, const char *what, int32_t n_outer, const int64_t *outer_shape, const int64_t *const (&outer_strides)[NS],
                          SliceLevels<NS> &kept, int64_t &rows, int32_t n_inner = 0, const int64_t *inner_shape = nullptr,
                          const int64_t *inner_strides = nullptr, SliceLevels<1> *red = nullptr, int *inner = nullptr) {
    bool ok = n_outer >= 0 && n_outer <= SLICE_MAX_LEVELS && n_inner >= 0 && n_inner <= SLICE_MAX_LEVELS && (!n_outer || outer_shape) &&
              (!n_inner || (inner_shape && inner_strides));
    for (int s = 0; s < NS; s++) ok = ok && (!n_outer || outer_strides[s]);
    if (!ok) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, red ? "%s: at most 6 kept and 6 reduced dims" : "%s: at most 6 kept dims", what);
    kept = SliceLevels<NS>{};
    kept.n = n_outer;
    rows = 1;
    for (int d = 0; d < n_outer; d++) {
        bool dim_ok = outer_shape[d] >= 0 && outer_shape[d] <= 0x7fffffff;
        for (int s = 0; s < NS; s++) dim_ok = dim_ok && outer_strides[s][d] >= 0;
        if (!dim_ok) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "%s: bad dimension", what);
        kept.shape[d] = (int32_t)outer_shape[d];
        for (int s = 0; s < NS; s++) kept.stride[s][d] = outer_strides[s][d];
        rows *= outer_shape[d];
    }
    if (!red) return RTEN_HIP_OK;
    *red = SliceLevels<1>{};
    red->n = n_inner > 0 ? n_inner : 1;
    red->shape[0] = 1;
    int64_t len = 1;
    for (int d = 0; d < n_inner; d++) {
        if (inner_shape[d] < 0 || inner_strides[d] < 0) return rten_set_error(ctx, RTEN_HIP_ERR_INVALID_VALUE, "%s: bad dimension", what);
        len *= inner_shape[d];
        if (len > 0x7fffffff) return rten_set_error(ctx, RTEN_HIP_ERR_UNSUPPORTED, "%s: reduced slice longer than 2^31 - 1", what);
        red->shape[d] = (int32_t)inner_shape[d];
        red->stride[0][d] = inner_strides[d];
    }
    *inner = (int)len;
    return RTEN_HIP_OK;
}
