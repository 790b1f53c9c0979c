// Host-side check of the strided reductions' addressing (slice_row_bases / slice_row_base / slice_elem_off, rten_amd/csrc/slice.h): the SAME functions, compiled for the
// host by hipcc (no GPU needed), against a naive unravel-and-dot-product.  Only offsets are computed: no memory is touched.
#include "../../rten_amd/csrc/slice.h"

#include <cstdio>
#include <vector>

static long long bad = 0, checked = 0;

// row-major unravel of `index` over `shape`, dotted with `stride`
static int64_t naive(int n, const int32_t *shape, const int64_t *stride, int64_t index) {
    int64_t coord[SLICE_MAX_LEVELS] = {0};
    for (int d = n - 1; d >= 0; d--) {
        coord[d] = index % shape[d];
        index /= shape[d];
    }
    int64_t off = 0;
    for (int d = 0; d < n; d++) off += coord[d] * stride[d];
    return off;
}

static void expect(int64_t got, int64_t want, const char *what, int n, int64_t index) {
    checked++;
    if (got != want && bad++ < 8) std::printf("mismatch: %s, %d levels, index %lld: %lld, expected %lld\n", what, n, (long long)index, (long long)got, (long long)want);
}

int main() {
    const int32_t extents[] = {1, 2, 3, 7, 16};
    // zero (a broadcast dim), non-monotone and large strides; the second list shares the shape (TopK's output strides)
    const int64_t strides_a[] = {0, 5, 1, 1000003, 12, 7, 0, 3, 4096, 1, 77};
    const int64_t strides_b[] = {9, 0, 640, 2, 1, 33, 100000007, 0, 8, 5, 6};
    unsigned seed = 12345;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int n = 0; n <= SLICE_MAX_LEVELS; n++) {
        for (int trial = 0; trial < 200; trial++) {
            SliceLevels<2> kept = {};
            SliceLevels<1> red = {};
            kept.n = n;
            red.n = n ? n : 1; // the entry points pass no reduced dims as one level of one element
            red.shape[0] = 1;
            int64_t count = 1;
            for (int d = 0; d < n; d++) {
                kept.shape[d] = red.shape[d] = extents[(trial < 5 ? (unsigned)trial : next()) % 5];
                kept.stride[0][d] = red.stride[0][d] = strides_a[next() % 11];
                kept.stride[1][d] = strides_b[next() % 11];
                count *= kept.shape[d];
            }
            for (int64_t i = 0; i < count; i++) {
                int64_t both[2];
                slice_row_bases(kept, count, i, both);
                expect(both[0], naive(n, kept.shape, kept.stride[0], i), "row_bases (first stride list)", n, i);
                expect(both[1], naive(n, kept.shape, kept.stride[1], i), "row_bases (second stride list)", n, i);
                expect(slice_row_base(red, count, i), both[0], "row_base", n, i);
                expect(slice_elem_off(red, (int)i), naive(n, red.shape, red.stride[0], i), "elem_off", n, i);
            }
        }
    }
    // more than 2^31 rows, which takes two levels at least: the 64-bit branch
    for (int n = 2; n <= SLICE_MAX_LEVELS; n++) {
        SliceLevels<1> kept = {};
        kept.n = n;
        int64_t below = 1;
        for (int d = 1; d < n; d++) {
            kept.shape[d] = extents[(d + n) % 5];
            kept.stride[0][d] = strides_a[(3 * d + n) % 11];
            below *= kept.shape[d];
        }
        kept.shape[0] = (int32_t)(((1LL << 31) + 5 + below - 1) / below);
        kept.stride[0][0] = 1000003;
        const int64_t rows = kept.shape[0] * below;
        if (rows <= 0x7fffffff) { std::printf("the large case is not large\n"); return 1; }
        for (int64_t row : {(int64_t)0, (int64_t)1, below, (int64_t)0x7fffffff, (int64_t)0x80000000LL, rows / 2 + 3, rows - 2, rows - 1})
            expect(slice_row_base(kept, rows, row), naive(n, kept.shape, kept.stride[0], row), "row_base (64-bit)", n, row);
    }
    std::printf("%lld offsets checked, %lld mismatches\n", checked, bad);
    return bad ? 1 : 0;
}
