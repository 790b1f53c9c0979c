"""What a kernel may touch: helpers for the two properties tests/test_gpu_confine.py checks on every entry point.

1. A kernel writes exactly the elements of its output.  `Guarded` puts a tensor into ONE device allocation laid out as

       [ front guard | lead bytes | region | back guard ]

   that is filled with one byte value before the region is uploaded; after the launch `assert_confined` demands that every byte
   outside the written elements (guards, the lead, and the gaps a strided output leaves: `ldc > n`, a batch stride with slack, a
   destination row stride) still holds the fill.  The default fill 0xFF is, read as float32, a NaN no kernel here produces and,
   read as int32, -1.  Outputs of 8-bit types are run once per value of `FILLS_8BIT`: a stray saturated code (0xFF) cannot hide
   in both.
2. An element outside an operand, or inside it but unrelated to an output element, cannot influence that element.  Inputs go
   through `Guarded` too (fill 0xFF): a lane that reads past an operand and lets the value reach the output turns it into a NaN,
   which fails the bit comparison with the oracle.  The `*_nonfinite` builders put NaN / Inf at stated places INSIDE the operands;
   tests/test_confine.py asserts on the CPU that the oracle confines each of them to the stated dependency set, the GPU tests then
   compare with the oracle.

Guard sizes are a condition, not a measurement: a guard must be large enough that the furthest plausible stray store of the
kernel under test still lands in it.
  * flat and row-wise kernels (one lane or one workgroup per run of elements): `GUARD_FLAT` = 64 KiB in front and behind;
  * tiled kernels: one full tile past the output in both directions.  The largest tile is 128 x 128, so for a GEMM that is
    `gemm_guard(ldc)` = 128 * ldc + 128 elements (128 rows further down plus 128 columns further right), for an NCHW output
    `nchw_guard(plane)` = 128 channels x plane elements.
Both are computed per case; nothing smaller than `GUARD_FLAT` is ever used, so the tiled rule only ever widens a guard.

The module is plain numpy apart from `Guarded` (which needs a context): `assert_confined` and the mask builders are tested
without a GPU."""
import numpy as np

FILL = 0xFF
FILLS_8BIT = (0xFF, 0x5A)
GUARD_FLAT = 64 * 1024  # bytes
F = np.float32


def round_up(v, to):
    return (int(v) + to - 1) // to * to


def gemm_guard(ldc, itemsize=4):
    """Bytes of one full 128 x 128 tile past a matrix with row stride `ldc` (never below GUARD_FLAT)."""
    return max(GUARD_FLAT, round_up((128 * int(ldc) + 128) * itemsize, 16))


def nchw_guard(plane, itemsize=4):
    """Bytes of 128 channels of `plane` elements (a tile's rows are output channels; never below GUARD_FLAT)."""
    return max(GUARD_FLAT, round_up(128 * int(plane) * itemsize, 16))


def span(shape, strides):
    """Elements from the first to one past the last element of a strided tensor (strides in elements, all >= 0)."""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((n - 1) * st for n, st in zip(shape, strides))


def strided_mask(total, region, itemsize, shape, strides):
    """Boolean byte mask of a whole allocation of `total` bytes: True on the bytes of the elements of a tensor of `shape` /
    `strides` (elements) whose first element sits `region` bytes into the allocation."""
    mask = np.zeros(total, bool)
    if any(s == 0 for s in shape):
        return mask
    idx = np.zeros((), np.int64)
    for n, st in zip(shape, strides):
        idx = idx[..., None] + np.arange(n, dtype=np.int64) * int(st)
    start = region + idx.reshape(-1) * itemsize
    assert start.min() >= 0 and start.max() + itemsize <= total, "the tensor does not fit the allocation"
    for b in range(itemsize):
        mask[start + b] = True
    return mask


def locate(rel_byte, itemsize, strides):
    """Index, in the caller's axis order, of the element a byte offset relative to the region falls into, for a layout of `strides` (elements, any
    order, 0 = an axis of extent 1): the offset is taken apart from the largest stride down."""
    e = rel_byte // itemsize
    at = [0] * len(strides)
    for ax in sorted(range(len(strides)), key=lambda a: -strides[a]):
        if strides[ax]:
            at[ax] = int(e // strides[ax])
            e -= at[ax] * strides[ax]
    return tuple(at)


def assert_confined(raw, written, fill, what, region=0, itemsize=1, strides=None, axes=None):
    """Every byte of `raw` (the whole allocation as uint8) outside the boolean byte mask `written` must equal `fill`.  The message
    names the first offending byte relative to `region` (the byte offset of the output's first element) and, with `strides`
    (elements, in the output's own axis order) and `axes` (their names), as an index of that layout, e.g. batch 1, row 2, column 8."""
    raw = np.asarray(raw).view(np.uint8).reshape(-1)
    written = np.asarray(written, bool).reshape(-1)
    assert raw.size == written.size, (what, raw.size, written.size)
    bad = (raw != fill) & ~written
    if not bad.any():
        return
    first = int(np.flatnonzero(bad)[0])
    rel = first - region
    where = "front guard" if rel < 0 else "back guard / gap"
    msg = f"{what}: {int(bad.sum())} bytes outside the output were written; first at byte {rel:+d} relative to the output ({where}): " \
          f"0x{int(raw[first]):02x} instead of the fill 0x{fill:02x}"
    if strides is not None and rel >= 0:
        names = axes if axes is not None else [f"axis{i}" for i in range(len(strides))]
        at = ", ".join(f"{nm} {v}" for nm, v in zip(names, locate(rel, itemsize, strides)))
        msg += f", element ({at}) of the layout with strides {tuple(int(s) for s in strides)}"
    raise AssertionError(msg)


class Guarded:
    """One device allocation `[front guard | lead | region | back guard]`, every byte `fill` except the region, which holds
    `nbytes_or_array` (an array: uploaded; a byte count: left at the fill -- an output).  `lead` is in elements of the dtype
    (`itemsize` when only a byte count is given) and moves the region off its 16-byte boundary; `front` / `back` are bytes (the
    front guard is rounded up to 16 so that `lead` alone decides the region's alignment)."""

    def __init__(self, ctx, nbytes_or_array, lead=0, front=GUARD_FLAT, back=GUARD_FLAT, fill=FILL, itemsize=4):
        from rten_amd.tensor import DeviceTensor
        self.ctx, self.fill = ctx, fill
        if isinstance(nbytes_or_array, (int, np.integer)):
            data, self.nbytes = None, int(nbytes_or_array)
        else:
            data = np.ascontiguousarray(nbytes_or_array)
            itemsize = data.dtype.itemsize
            self.nbytes = data.nbytes
            data = data.reshape(-1).view(np.uint8)
        self.region = round_up(front, 16) + lead * itemsize
        self.total = self.region + self.nbytes + int(back)
        host = np.full(self.total, fill, np.uint8)
        if data is not None:
            host[self.region:self.region + self.nbytes] = data
        self.buf = DeviceTensor.from_numpy(ctx, host)
        assert self.buf.ptr % 16 == 0
        self.ptr = self.buf.ptr + self.region

    @property
    def vp(self):
        import ctypes
        return ctypes.c_void_p(self.ptr)

    def tensor(self, shape, dtype=np.float32):
        from rten_amd.tensor import DeviceTensor
        return DeviceTensor(self.ctx, shape, dtype, ptr=self.ptr, keepalive=self.buf)

    def fill_region(self, arr):
        """Upload `arr` (bytes of the region's prefix) without touching the guards: an output pre-filled for beta != 0 / in place."""
        from rten_amd.tensor import DeviceTensor
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        DeviceTensor(self.ctx, (arr.nbytes,), np.uint8, ptr=self.ptr, keepalive=self.buf).upload(arr.reshape(-1).view(np.uint8))

    def raw(self):
        """The whole allocation as uint8."""
        return self.buf.numpy()

    def strided(self, raw, shape, strides, dtype=np.float32):
        """The tensor of `shape` / `strides` (elements) at the region, cut out of `raw`, as a contiguous array."""
        dtype = np.dtype(dtype)
        n = span(shape, strides)
        flat = raw[self.region:self.region + n * dtype.itemsize].view(dtype)
        return np.ascontiguousarray(np.lib.stride_tricks.as_strided(flat, shape, [s * dtype.itemsize for s in strides]))

    def check(self, raw, shape, strides, dtype, what, axes=None):
        """assert_confined for an output of `shape` / `strides` (elements) at the region, `axes` naming its axes in the message; -> its contents."""
        dtype = np.dtype(dtype)
        assert span(shape, strides) * dtype.itemsize <= self.nbytes, "the region is smaller than the output's span"
        written = strided_mask(self.total, self.region, dtype.itemsize, shape, strides)
        assert_confined(raw, written, self.fill, what, self.region, dtype.itemsize, strides, axes)
        return self.strided(raw, shape, strides, dtype)


def dense(shape):
    """Row-major strides (elements) of `shape`."""
    st, acc = [], 1
    for n in reversed(shape):
        st.append(acc)
        acc *= max(int(n), 1)
    return tuple(reversed(st))


def bits_equal(got, want, what=""):
    """The rule of tests/test_gpu_parity.py (float32: +0 == -0, NaNs must coincide, everything else the same bits -- no tolerance; integer types:
    equality), with the case named in the message and the dtype checked first."""
    from tests.test_gpu_parity import bits_equal as parity_bits_equal
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    try:
        with np.errstate(invalid="ignore"):
            parity_bits_equal(got, want)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


# ------------------------------------------------------------------------------------------------ non-finite inputs and what depends on them
def gemm_nonfinite(a, b):
    """A row 5 all NaN, A[m-1, k-1] = +Inf, B column 7 all NaN, B[k-1, n-1] = -Inf -> (a, b, dependency mask [m, n]): rows 5 and
    m-1 and columns 7 and n-1 depend on a non-finite value, nothing else does."""
    a, b = a.copy(), b.copy()
    m, n = a.shape[0], b.shape[1]
    assert m > 6 and n > 8
    a[5, :] = np.nan
    a[m - 1, -1] = np.inf
    b[:, 7] = np.nan
    b[-1, n - 1] = -np.inf
    dep = np.zeros((m, n), bool)
    dep[[5, m - 1], :] = True
    dep[:, [7, n - 1]] = True
    return a, b, dep


def conv_dependency(xmask, wshape, pads, strides, dilations=(1, 1), groups=1):
    """Output elements [N, O, oh, ow] whose receptive field holds a marked input element (every weight taken as non-zero): the
    window arithmetic of a convolution written out tap by tap."""
    n, c, h, w = xmask.shape
    o, cg, kh, kw = wshape
    pt, pl, pb, pr = pads
    oh = (h + pt + pb - dilations[0] * (kh - 1) - 1) // strides[0] + 1
    ow = (w + pl + pr - dilations[1] * (kw - 1) - 1) // strides[1] + 1
    og = o // groups
    dep = np.zeros((n, o, oh, ow), bool)
    for g in range(groups):
        any_c = xmask[:, g * cg:(g + 1) * cg].any(axis=1)  # [n, h, w]
        hit = np.zeros((n, oh, ow), bool)
        for ky in range(kh):
            for kx in range(kw):
                for oy in range(oh):
                    iy = oy * strides[0] - pt + ky * dilations[0]
                    if not 0 <= iy < h:
                        continue
                    ix = np.arange(ow) * strides[1] - pl + kx * dilations[1]
                    ok = (ix >= 0) & (ix < w)
                    hit[:, oy, ok] |= any_c[:, iy, ix[ok]]
        dep[:, g * og:(g + 1) * og] = hit[:, None]
    return dep


def conv_nonfinite(x):
    """Image 1 all NaN, +Inf at the last pixel of the last channel of the last image (in memory its successor is the guard), -Inf at
    pixel (0, 0) of channel 0 of image 0 -> (x, mask of the non-finite input elements)."""
    x = x.copy()
    assert x.shape[0] >= 2
    x[1] = np.nan
    x[-1, -1, -1, -1] = np.inf
    x[0, 0, 0, 0] = -np.inf
    return x, ~np.isfinite(x)


def rows_nonfinite(x):
    """[rows >= 5, cols]: row 1 all NaN, row 2 holds +Inf, row 3 holds -Inf among finite values -> (x, rows that depend on them)."""
    x = x.copy()
    assert x.shape[0] >= 5
    x[1] = np.nan
    x[2, x.shape[1] // 2] = np.inf
    x[3, -1] = -np.inf
    dep = np.zeros(x.shape[0], bool)
    dep[1:4] = True
    return x, dep


# ------------------------------------------------------------------------------------------------ the non-finite cases both test files use
GEMM_NONFINITE_SHAPES = [(65, 257, 129), (130, 520, 264)]  # (m, k, n): one past a tile / depth block everywhere; several ragged tiles, three depth blocks
# n, c, h, w, o, kh, kw, pads, strides, dilations, groups
CONV_NONFINITE_CASES = {
    "generic-k72": (2, 8, 11, 13, 70, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 1),
    "generic-k270-s2": (2, 30, 11, 13, 70, 3, 3, (1, 1, 1, 1), (2, 2), (1, 1), 1),
    "pointwise": (3, 64, 7, 7, 70, 1, 1, (0, 0, 0, 0), (1, 1), (1, 1), 1),
    "stem": (2, 3, 37, 41, 24, 7, 7, (3, 3, 3, 3), (2, 2), (1, 1), 1),
    "grouped": (2, 8, 11, 13, 6, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 2),
    "depthwise": (2, 5, 6, 10, 5, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 5),
}
ROWS_NONFINITE_COLS = [17, 257]  # rows = 5


def seeded(shape, seed, scale=1.0):
    """Seeded float32 values in (-0.5, 0.5) * scale from the oracle's generator."""
    from oracle import ref
    n = int(np.prod(shape))
    return ((ref.XorShiftRng(seed).f32(n).reshape(shape) - F(0.5)) * F(scale)).astype(F)


def conv_operands(case, seed=4321):
    n, c, h, w, o, kh, kw, pads, strides, dil, groups = case
    x = seeded((n, c, h, w), seed)
    wt = seeded((o, c // groups, kh, kw), seed + 1, 0.5)
    b = seeded((o,), seed + 2)
    return x, wt, b


def sdpa_operands(b, h, s, t, d, seed=99):
    return seeded((b, h, s, d), seed), seeded((b, h, t, d), seed + 1), seeded((b, h, t, d), seed + 2)


def sdpa_nonfinite(k):
    """A NaN row (key 2, or the only key) in K of (batch 1, head 0): only out[1, 0] may change."""
    k = k.copy()
    k[1, 0, min(2, k.shape[2] - 1), :] = np.nan
    return k


def sdpa_trailing_mask(b, t, masked):
    """[B, 1, 1, T] additive mask: batch 0 has -inf on its last `masked` keys (padding of a shorter sequence), the others 0."""
    m = np.zeros((b, 1, 1, t), F)
    m[0, 0, 0, t - masked:] = -np.inf
    return m


def pool_nonfinite(x, value):
    """`value` at the corner pixel (0, 0) of plane (0, 0): only output pixel (0, 0) of that plane sees it."""
    x = x.copy()
    x[0, 0, 0, 0] = value
    return x
