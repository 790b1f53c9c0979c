"""numpy restatements of the reference's GridSample (src/ops/grid_sample.rs:12-125) and DepthToSpace (src/ops/layout.rs:28-66): the rules the
host layers, the kernel and the graph executor are checked against.  Test infrastructure only.

grid_sample is vectorised over pixels and channels; every arithmetic step is ONE float32 operation on float32 arrays (numpy rounds each to nearest
even, as the reference's scalar code does), and `floor(s) as i32` is Rust's cast: saturating, NaN -> 0."""
import numpy as np

F = np.float32
I32_MAX, I32_MIN = 2**31 - 1, -2**31


def rust_f32_as_i32(f):
    """`f as i32` on a float32 array -> int64 array holding the i32 values."""
    f = np.asarray(f, F)
    with np.errstate(invalid="ignore"):
        t = np.where(np.isnan(f), F(0), f)
        t = np.clip(t.astype(np.float64), float(I32_MIN), float(I32_MAX))
        return np.trunc(t).astype(np.int64)


def _axis(g, length, align_corners):
    """One coordinate axis: (i0, i1, w) = (floor(s) as i32, its neighbour, s - floor(s)), grid_sample.rs:59-93."""
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((g + F(1)).astype(F) * F(0.5)).astype(F)
        if align_corners:
            s = ((F(length) - F(1)).astype(F) * u).astype(F)
        else:
            s = ((F(length) * u).astype(F) - F(0.5)).astype(F)
        fl = np.floor(s).astype(F)
        w = (s - fl).astype(F)
    i0 = rust_f32_as_i32(fl)
    return i0, i0 + 1, w  # (at i32::MAX the release build wraps to i32::MIN and a 64-bit sum gives 2^31: out of bounds either way)


def _lerp(a, b, w):
    with np.errstate(invalid="ignore", over="ignore"):
        return (a + ((b - a).astype(F) * w).astype(F)).astype(F)


def grid_sample(x, grid, align_corners=False):
    x, grid = np.asarray(x, F), np.asarray(grid, F)
    n, c, in_h, in_w = x.shape
    gn, out_h, out_w, two = grid.shape
    assert gn == n and two == 2
    y = np.zeros((n, c, out_h, out_w), F)
    if in_h == 0 or in_w == 0 or y.size == 0:
        return y
    x0, x1, wx = _axis(grid[..., 0], in_w, align_corners)  # [n, out_h, out_w]
    y0, y1, wy = _axis(grid[..., 1], in_h, align_corners)
    b = np.arange(n)[:, None, None, None]
    ch = np.arange(c)[None, :, None, None]

    def pixel(iy, ix):
        ok = (iy >= 0) & (iy < in_h) & (ix >= 0) & (ix < in_w)
        v = x[b, ch, np.where(ok, iy, 0)[:, None], np.where(ok, ix, 0)[:, None]]
        return np.where(ok[:, None], v, F(0)).astype(F)  # +0.0 outside; the value at the clamped address is dropped

    wx, wy = wx[:, None], wy[:, None]
    top = _lerp(pixel(y0, x0), pixel(y0, x1), wx)
    bottom = _lerp(pixel(y1, x0), pixel(y1, x1), wx)
    return _lerp(top, bottom, wy)


def footprint(grid, in_h, in_w, align_corners=False):
    """For every output pixel the set of in-bounds input pixels its 2x2 neighbourhood holds, zero-weight neighbours included:
    a bool array [n, out_h, out_w, in_h, in_w]."""
    grid = np.asarray(grid, F)
    x0, x1, _ = _axis(grid[..., 0], in_w, align_corners)
    y0, y1, _ = _axis(grid[..., 1], in_h, align_corners)
    hit = np.zeros(grid.shape[:3] + (in_h, in_w), bool)
    idx = np.indices(grid.shape[:3])
    for iy in (y0, y1):
        for ix in (x0, x1):
            ok = (iy >= 0) & (iy < in_h) & (ix >= 0) & (ix < in_w)
            hit[idx[0][ok], idx[1][ok], idx[2][ok], iy[ok], ix[ok]] = True
    return hit


DEPTH_TO_SPACE = {"DCR": (lambda n, b, c, h, w: (n, b, b, c, h, w), (0, 3, 4, 1, 5, 2)), "CRD": (lambda n, b, c, h, w: (n, c, b, b, h, w), (0, 1, 4, 2, 5, 3))}


def depth_to_space(x, block_size, mode="DCR"):
    """layout.rs:28-66: the reshape / permute / reshape of the ONNX specification."""
    x = np.asarray(x)
    n, c, h, w = x.shape
    b = int(block_size)
    assert b > 0 and c % (b * b) == 0
    view, perm = DEPTH_TO_SPACE[mode]
    nc = c // (b * b)
    return np.ascontiguousarray(x.reshape(view(n, b, nc, h, w)).transpose(perm)).reshape(n, nc, h * b, w * b)
