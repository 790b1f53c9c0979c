"""Where a kernel writes and what it may read (docs/KERNELS.md 4.10), on the device, through the C ABI.

Every case runs an entry point into a `tests.confine.Guarded` output (one allocation `[front guard | lead | output | back guard]`
filled with 0xFF), compares the written elements with the CPU oracle bit for bit, and demands that every byte outside the
output's elements -- guards, the lead and the gaps of a strided output -- still holds the fill.  Operands sit in 0xFF guards too
(as float32 a NaN): a lane that reads outside its operand and lets the value reach an output fails the bit comparison.  The
second half puts NaN / Inf INSIDE operands at places a subset of the outputs depends on; tests/test_confine.py asserts on the CPU
that the oracle confines them, here the device must give the oracle's bits.  No tolerance anywhere."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from oracle import ref
from rten_amd import lib as L
from tests import confine as K
from tests import norm_rules as NR

pytestmark = pytest.mark.gpu

F = np.float32


def kernels_of(ctx, fn):
    """Kernel names (the ProfScope strings of the sources) `fn` launched."""
    ctx.profile(True)
    ctx.profile_reset()
    try:
        fn()
        ctx.sync()
        return {e["kernel"] for e in ctx.profile_report()}
    finally:
        ctx.profile(False)
        ctx.profile_reset()


def guarded_in(ctx, arr, lead=0):
    return K.Guarded(ctx, arr, lead=lead)


# ================================================================================================ f32 GEMM: writes
GEMM_SHAPES = [(33, 17, 31),     # below a tile, k % 4 != 0
               (64, 256, 128),   # exact tiles: the unmasked fast path must not write an extra tile
               (65, 257, 129),   # one past a tile and one past a depth block in every dimension
               (130, 520, 264),  # several ragged tiles, three depth blocks
               (32, 600, 200),   # the automatic small-M kernel
               (1, 300, 130),    # the gemv path
               (2, 1030, 5)]     # small m, long K
SPLIT_SHAPES = [(65, 257, 129), (130, 520, 264)]
SPLIT_VARIANTS = [0, 3, 20, 24, 27, 28, 31]
SPLIT_PLANS = [(0, 1), (2, 2), (2, 3), (2, 64), (1, 4), (5, 2)]
NUM_VARIANTS = 33  # rten_hip_num_gemm_variants(), asserted below (parametrisation happens before a context exists)
VARIANTS = [-1] + list(range(NUM_VARIANTS))  # -1: the automatic choice (small-M streaming, gemv, the cost model's tile)


def placements(n):
    """(ldc, element offset of C from a 16-byte boundary)"""
    return [(n, 0), (n, 2), (n + 1, 1), (n + 5, 3), (K.round_up(n, 4) + 4, 0)]


@functools.lru_cache(maxsize=None)
def gemm_operands(m, k, n, batch=1):
    a = K.seeded((batch, m, k), 1000 + m + k)
    b = K.seeded((batch, k, n), 2000 + k + n)
    c0 = K.seeded((batch, m, n), 3000 + m + n)
    return a, b, c0, K.seeded((m,), 17), K.seeded((n,), 19)


EPILOGUES = ["plain", "beta1", "row-bias-relu", "col-bias-gelu", "act-sigmoid"]


@functools.lru_cache(maxsize=None)
def gemm_want(m, k, n, epilogue, batch=1, b_t=False):
    """The oracle on the operands as laid out (it honours strides): a one-row product takes the reference's vector-matrix kernels, whose order
    depends on whether B's rows or columns are contiguous; for m > 1 the layout does not change a bit."""
    a, b, c0, br, bc = gemm_operands(m, k, n, batch)
    if b_t:
        b = np.ascontiguousarray(b.transpose(0, 2, 1)).transpose(0, 2, 1)
    out = []
    for z in range(batch):
        if epilogue == "plain":
            y = ref.gemm_f32(a[z], b[z])
        elif epilogue == "beta1":
            y = ref.gemm_f32(a[z], b[z], c=c0[z], alpha=0.5, beta=1.0)
        elif epilogue == "row-bias-relu":
            y = ref.relu(ref.gemm_f32(a[z], b[z], bias=br, bias_kind=ref.BIAS_PER_ROW))
        elif epilogue == "col-bias-gelu":
            y = ref.gelu(ref.gemm_f32(a[z], b[z], bias=bc, bias_kind=ref.BIAS_PER_COL))
        else:
            y = NR.activation(L.ACT_SIGMOID, ref.gemm_f32(a[z], b[z]))
        out.append(y)
    return np.stack(out)


class GemmCase:
    """One product's operands on the device (in guards, uploaded once) and launches of it into guarded outputs."""

    def __init__(self, ctx, m, k, n, batch=1, a_t=False, b_t=False, a=None, b=None):
        self.ctx, self.m, self.k, self.n, self.batch = ctx, m, k, n, batch
        ops = gemm_operands(m, k, n, batch)
        a = ops[0] if a is None else a
        b = ops[1] if b is None else b
        self.c0, self.br, self.bc = ops[2], ops[3], ops[4]
        # transposed operands are strides: the same logical matrix stored column-major
        self.a_g = guarded_in(ctx, np.ascontiguousarray(a.transpose(0, 2, 1)) if a_t else a)
        self.b_g = guarded_in(ctx, np.ascontiguousarray(b.transpose(0, 2, 1)) if b_t else b)
        self.b_t = b_t
        self.a_st = (1, m) if a_t else (k, 1)
        self.b_st = (1, k) if b_t else (n, 1)
        self.br_g, self.bc_g = guarded_in(ctx, self.br), guarded_in(ctx, self.bc)

    def run(self, ldc, lead, epilogue="plain", want=None, what="", c_bs=None, inner=None):
        """`inner` = (batch_inner, c_bsi): the two-level batch; A and B batches stay dense."""
        ctx, m, k, n, batch = self.ctx, self.m, self.k, self.n, self.batch
        c_bs = m * ldc if c_bs is None else c_bs
        if inner:
            bi, c_bsi = inner
            shape, strides = (batch // bi, bi, m, n), (c_bs, c_bsi, ldc, 1)
        else:
            bi, c_bsi = 0, 0
            shape, strides = (batch, m, n), (c_bs, ldc, 1)
        guard = K.gemm_guard(ldc)
        nbytes = 4 * K.span(shape, strides)
        out = K.Guarded(ctx, nbytes, lead=lead, front=guard, back=guard)
        alpha, beta, bias, kind, act = 1.0, 0.0, None, L.BIAS_NONE, L.ACT_NONE
        if epilogue == "beta1":  # C is read through ldc: its elements are pre-filled, the gaps keep the fill pattern
            alpha, beta = 0.5, 1.0
            host = np.full(nbytes, K.FILL, np.uint8)
            np.lib.stride_tricks.as_strided(host.view(F), shape, [4 * s for s in strides])[...] = self.c0.reshape(shape)
            out.fill_region(host)
        elif epilogue == "row-bias-relu":
            bias, kind, act = self.br_g, L.BIAS_PER_ROW, L.ACT_RELU
        elif epilogue == "col-bias-gelu":
            bias, kind, act = self.bc_g, L.BIAS_PER_COL, L.ACT_GELU
        d = L.gemm_desc(m, n, k, *self.a_st, *self.b_st, ldc, batch=batch, a_bs=m * k, b_bs=k * n, c_bs=c_bs, alpha=alpha, beta=beta,
                        bias_kind=kind, act=act, batch_inner=bi, a_bsi=m * k if inner else 0, b_bsi=k * n if inner else 0, c_bsi=c_bsi)
        if inner:
            d.a_bs, d.b_bs = bi * m * k, bi * k * n
        if epilogue == "act-sigmoid":
            ctx.call("rten_hip_gemm_f32_act", C.byref(d), self.a_g.vp, self.b_g.vp, None, L.ACT_SIGMOID, 0.0, 0.0, out.vp)
        else:
            ctx.call("rten_hip_gemm_f32", C.byref(d), self.a_g.vp, self.b_g.vp, None if bias is None else bias.vp, out.vp)
        ctx.sync()
        what = f"gemm {m}x{k}x{n} {epilogue} ldc {ldc} lead {lead} {what}"
        got = out.check(out.raw(), shape, strides, F, what, ("batch", "inner batch", "row", "column") if inner else ("batch", "row", "column"))
        want = gemm_want(m, k, n, epilogue, batch, self.b_t and m == 1) if want is None else want
        K.bits_equal(got, want.reshape(shape), what)


class knobs:
    """GEMM variant / split plan / tile order for a block, restored afterwards."""

    def __init__(self, ctx, variant=-1, split=(3, 1), order=0):
        self.ctx, self.variant, self.split, self.order = ctx, variant, split, order

    def __enter__(self):
        self.ctx.set_gemm_variant(self.variant)
        self.ctx.call("rten_hip_set_gemm_split", *self.split)
        self.ctx.call("rten_hip_set_gemm_order", self.order)

    def __exit__(self, *exc):
        self.ctx.set_gemm_variant(-1)
        self.ctx.call("rten_hip_set_gemm_split", 3, 1)
        self.ctx.call("rten_hip_set_gemm_order", 0)


def test_variant_count(ctx):
    assert ctx.lib.rten_hip_num_gemm_variants() == NUM_VARIANTS


@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_every_variant_shape_and_placement(ctx, variant):
    """The full cross under the default split plan: 7 shapes x 5 placements of C per variant."""
    with knobs(ctx, variant):
        for (m, k, n) in GEMM_SHAPES:
            case = GemmCase(ctx, m, k, n)
            for ldc, lead in placements(n):
                case.run(ldc, lead, what=f"variant {variant}")


@pytest.mark.parametrize("variant", SPLIT_VARIANTS)
def test_gemm_split_plans_and_tile_orders(ctx, variant):
    for (m, k, n) in SPLIT_SHAPES:
        case = GemmCase(ctx, m, k, n)
        for split in SPLIT_PLANS:
            for order in range(4):
                with knobs(ctx, variant, split, order):
                    for ldc, lead in ((n + 1, 1), (K.round_up(n, 4) + 4, 0)):
                        case.run(ldc, lead, what=f"variant {variant} split {split} order {order}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_epilogues(ctx, variant):
    """beta = 1 reads C through ldc (the gaps keep the pattern, so a read of a gap element would poison the row), bias per row and
    per column with the fused activations, and the _act entry point; also under a split plan, whose fold runs the same epilogue."""
    for (m, k, n) in SPLIT_SHAPES + [(32, 600, 200)]:
        case = GemmCase(ctx, m, k, n)
        for split in ((3, 1), (2, 2)):
            with knobs(ctx, variant, split):
                for epilogue in EPILOGUES[1:]:
                    for ldc, lead in ((n + 5, 3), (K.round_up(n, 4) + 4, 0)):
                        case.run(ldc, lead, epilogue, what=f"variant {variant} split {split}")


LOADER_SHAPES = [(64, 256, 128), (130, 520, 264), (132, 264, 136)]  # the last: m % 4 == 0 (16-byte loads of a transposed A) with ragged tiles


@pytest.mark.parametrize("shape", LOADER_SHAPES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("a_t, b_t", [(False, False), (True, False), (False, True), (True, True)], ids=["nn", "tn", "nt", "tt"])
def test_gemm_operand_layouts_reach_every_family(ctx, a_t, b_t, shape):
    """The four row-major / transposed loader combinations on every variant, and the kernel families they reach: a sweep that fell back
    to one kernel everywhere fails here.  Names are the ProfScope strings of csrc/gemm_f32*.hip."""
    names = set()
    for (m, k, n) in (shape,):
        case = GemmCase(ctx, m, k, n, a_t=a_t, b_t=b_t)
        for variant in VARIANTS:
            for split in ((3, 1), (2, 2), (5, 2)):
                with knobs(ctx, variant, split):
                    names |= kernels_of(ctx, lambda: case.run(K.round_up(n, 4) + 4, 0, what=f"variant {variant} split {split} A^T {a_t} B^T {b_t}"))
                    case.run(n + 1, 1, what=f"variant {variant} split {split} A^T {a_t} B^T {b_t}")
    families = {re.match(r"[a-z0-9_]+", nm).group(0) for nm in names}
    split_producers = {nm for nm in names if re.fullmatch(r"igemm_f32_(dma_)?kernel<.*,2(,\d)?>", nm) or re.fullmatch(r"igemm_f32_wave_kernel<\d+,2,\d+>", nm)}
    print(sorted(names))
    m, k, n = shape
    want = {"igemm_f32_kernel"}  # register-staged: every layout
    if m <= 64:
        want.add("gemm_f32_smallm_kernel")  # small-M streaming (the automatic choice and variant 31)
    a16 = m % 4 == 0 if a_t else k % 4 == 0  # the operand's contiguous extent is a whole number of 16-byte groups
    if not b_t and a16:
        # 16-byte loader pairs exist for (k-major A | row-major A) x row-major B: LDS-DMA, 16x16x4 MFMAs, the persistent walk
        want |= {"igemm_f32_dma_kernel", "igemm_f32_dma16_kernel", "igemm_f32_pers_kernel"}
        if a_t:
            want |= {"igemm_f32_ws_kernel", "igemm_f32_wave_kernel"}  # these take k-major A (the prepacked-weight layout) only
    assert families >= want, (sorted(want - families), sorted(names))
    if k > 256:  # (only depth-block boundaries are legal K cuts)
        assert split_producers, sorted(names)  # MODE 2 producers ran: the last-arrival fold wrote those tiles


def test_gemm_small_m_and_one_row_kernels_are_reached(ctx):
    names = set()
    for (m, k, n) in ((32, 600, 200), (2, 1030, 5), (1, 300, 130)):
        for b_t in (False, True):
            case = GemmCase(ctx, m, k, n, b_t=b_t)
            for ldc, lead in placements(n):
                for epilogue in EPILOGUES:
                    names |= kernels_of(ctx, lambda: case.run(ldc, lead, epilogue, what=f"automatic, B^T {b_t}"))
    assert names >= {"gemm_f32_smallm_kernel<2>", "gemm_f32_smallm_kernel<1>", "gemv_cols_kernel", "gemv_transposed_kernel"}, sorted(names)


@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_batches_write_their_own_slices(ctx, variant):
    """batch = 3 with slack between the C slices, and the Einsum layout: two batch levels whose inner products interleave column
    blocks of shared rows (ldc = H * n + 3, c_bsi = n, c_bs = m * ldc) -- each product writes only its own block."""
    for (m, k, n) in ((65, 257, 129), (33, 17, 31), (64, 256, 128)):
        case = GemmCase(ctx, m, k, n, batch=3)
        for split in ((3, 1), (2, 2)):
            with knobs(ctx, variant, split):
                for ldc, lead in ((n, 0), (n + 1, 1)):
                    case.run(ldc, lead, c_bs=m * ldc + 7, what=f"variant {variant} batch 3")
                case.run(n + 1, 1, "beta1", c_bs=m * (n + 1) + 7, what=f"variant {variant} batch 3")
        case = GemmCase(ctx, m, k, n, batch=4)
        H = 2
        ldc = H * n + 3
        with knobs(ctx, variant):
            for lead in (0, 1):
                case.run(ldc, lead, c_bs=m * ldc, inner=(H, n), what=f"variant {variant} two-level batch")
            case.run(ldc, 0, "col-bias-gelu", c_bs=m * ldc, inner=(H, n), what=f"variant {variant} two-level batch")


# ================================================================================================ f32 GEMM: non-finite operands
@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_nan_rows_and_columns_stay_in_their_rows_and_columns(ctx, variant):
    """A row 5 NaN, A[m-1, k-1] = +Inf, B column 7 NaN, B[k-1, n-1] = -Inf: the k-tail lanes, the padding rows and columns of the last
    tiles sit right beside them.  The oracle's result (tests/test_confine.py: non-finite exactly on rows 5, m-1 and columns 7, n-1, the
    all-finite bits elsewhere) is the expectation, default and (2, 3) split."""
    for (m, k, n) in K.GEMM_NONFINITE_SHAPES:
        a, b = gemm_operands(m, k, n)[:2]
        an, bn, dep = K.gemm_nonfinite(a[0], b[0])
        want = ref.gemm_f32(an, bn)
        assert np.array_equal(~np.isfinite(want), dep)
        for a_t in (False, True):
            case = GemmCase(ctx, m, k, n, a=an[None], b=bn[None], a_t=a_t)
            for split in ((3, 1), (2, 3)):
                with knobs(ctx, variant, split):
                    for ldc, lead in ((n, 0), (n + 1, 1), (K.round_up(n, 4) + 4, 0)):
                        case.run(ldc, lead, want=want[None], what=f"non-finite, variant {variant} split {split} A^T {a_t}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_nan_batch_slice_reaches_its_own_products_only(ctx, variant):
    m, k, n = 65, 257, 129
    a, b = gemm_operands(m, k, n, 4)[:2]
    an = a.copy()
    an[1] = np.nan
    want = np.stack([ref.gemm_f32(an[z], b[z]) for z in range(4)])
    assert np.isnan(want[1]).all() and np.isfinite(want[[0, 2, 3]]).all()
    case = GemmCase(ctx, m, k, n, batch=4, a=an)
    with knobs(ctx, variant):
        case.run(n + 1, 1, want=want, c_bs=m * (n + 1) + 7, what=f"NaN slice, variant {variant}")
        ldc = 2 * n + 3
        case.run(ldc, 0, want=want, c_bs=m * ldc, inner=(2, n), what=f"NaN slice, two-level, variant {variant}")


# ================================================================================================ f32 convolution
def conv_desc(case):
    n, c, h, w, o, kh, kw, pads, strides, dil, groups = case
    oh, ow, fp = ref.calc_output_size_and_padding((h, w), (kh, kw), strides, pads, dil)
    return L.Conv2dDesc(n, c, h, w, o, kh, kw, (C.c_int32 * 4)(*fp), strides[0], strides[1], dil[0], dil[1], groups, oh, ow), oh, ow


@functools.lru_cache(maxsize=None)
def conv_data(case, nonfinite=False):
    """-> x, w, bias, residual, want (bias only), want (bias + residual + Relu; all-finite inputs only)"""
    n, c, h, w, o, kh, kw, pads, strides, dil, groups = case
    x, wt, b = K.conv_operands(case)
    if nonfinite:
        x = K.conv_nonfinite(x)[0]
    plain = ref.conv2d_f32(x, wt, b, pads=pads, strides=strides, dilations=dil, groups=groups)
    res = K.seeded(plain.shape, 77)
    fused = None if nonfinite else ref.conv2d_f32(x, wt, b, pads=pads, strides=strides, dilations=dil, groups=groups, residual=res, relu=True)
    return x, wt, b, res, plain, fused


class ConvCase:
    """A convolution's operands in guards; the prepacked weights are written by rten_hip_conv2d_f32_prepack into a buffer of exactly
    rten_hip_conv2d_f32_packed_bytes() inside guards, which is checked as an output of its own."""

    def __init__(self, ctx, case, nonfinite=False, x_lead=0):
        self.ctx, self.case = ctx, case
        self.d, self.oh, self.ow = conv_desc(case)
        self.x, self.w, self.b, self.res, self.plain, self.fused = conv_data(case, nonfinite)
        self.x_g, self.w_g, self.b_g = guarded_in(ctx, self.x, x_lead), guarded_in(ctx, self.w), guarded_in(ctx, self.b)
        nbytes = ctx.lib.rten_hip_conv2d_f32_packed_bytes(C.byref(self.d))
        self.p_g = K.Guarded(ctx, nbytes)
        ctx.call("rten_hip_conv2d_f32_prepack", C.byref(self.d), self.w_g.vp, self.p_g.vp)
        ctx.sync()
        self.p_g.check(self.p_g.raw(), (nbytes // 4,), (1,), F, f"conv prepack {case}")

    def run(self, packed=True, fused=False, y_lead=0, res_lead=0, act=None, want=None, what=""):
        ctx, d = self.ctx, self.d
        n, o = self.case[0], self.case[4]
        shape = (n, o, self.oh, self.ow)
        guard = K.nchw_guard(self.oh * self.ow)
        out = K.Guarded(ctx, 4 * int(np.prod(shape)), lead=y_lead, front=guard, back=guard)
        res_g = guarded_in(ctx, self.res, res_lead) if fused else None
        wt = self.p_g if packed else self.w_g
        flags = L.CONV_RESIDUAL if fused else 0
        if act is not None:
            ctx.call("rten_hip_conv2d_f32_act", C.byref(d), self.x_g.vp, wt.vp, 1 if packed else 0, self.b_g.vp, None if res_g is None else res_g.vp, flags, act, 0.0, 0.0, out.vp)
        else:
            ctx.call("rten_hip_conv2d_f32", C.byref(d), self.x_g.vp, wt.vp, 1 if packed else 0, self.b_g.vp, None if res_g is None else res_g.vp,
                     flags | (L.CONV_RELU if fused else 0), out.vp)
        ctx.sync()
        what = f"conv {self.case} packed {packed} fused {fused} y+{y_lead} res+{res_lead} {what}"
        got = out.check(out.raw(), shape, K.dense(shape), F, what)
        K.bits_equal(got, (self.fused if fused else self.plain) if want is None else want, what)

    def both(self, what, leads=(1, 3)):
        """bias only at an aligned y; bias + residual + Relu with y and the residual off their 16-byte boundaries."""
        self.run(what=what)
        self.run(fused=True, y_lead=leads[0], res_lead=leads[1], what=what)


GENERIC = [(2, c, 11, 13, 70, 3, 3, (1, 1, 1, 1), (s, s), (1, 1), 1) for c in (8, 30) for s in (1, 2)]  # K = 72 and 270; 143 / 42 pixels per image
CONV_SPLITS = [(0, 1), (2, 2), (4, 1), (5, 2)]


@pytest.mark.parametrize("variant", VARIANTS)
def test_conv_generic_every_variant_and_split_mode(ctx, variant):
    for i, case in enumerate(GENERIC):
        cc = ConvCase(ctx, case)
        for split in CONV_SPLITS:
            with knobs(ctx, variant, split):
                cc.both(f"variant {variant} split {split}", leads=((1, 3), (3, 1))[i % 2])
        with knobs(ctx, variant):
            cc.run(packed=False, y_lead=3, what=f"variant {variant} plain OIHW weights")
            cc.run(act=L.ACT_SIGMOID, y_lead=1, want=NR.activation(L.ACT_SIGMOID, cc.plain), what=f"variant {variant} _act")


POINTWISE = [(3, 64, 7, 7, 70, 1, 1, (0, 0, 0, 0), (1, 1), (1, 1), 1),   # 147 columns, P = 49: the gather form
             (3, 64, 8, 8, 70, 1, 1, (0, 0, 0, 0), (1, 1), (1, 1), 1),   # P % 4 == 0: the dense two-level matrix
             (3, 32, 8, 8, 70, 1, 1, (0, 0, 0, 0), (1, 1), (1, 1), 1)]   # c = 32 for the lean persistent plan (mode 6)


@pytest.mark.parametrize("variant", VARIANTS)
def test_conv_pointwise_every_variant(ctx, variant):
    for case in POINTWISE:
        cc = ConvCase(ctx, case)
        for split in CONV_SPLITS + [(6, 2)]:
            with knobs(ctx, variant, split):
                cc.both(f"variant {variant} split {split}")


def test_conv_families_reached(ctx):
    """Kernel names of the convolution sweeps (ProfScope strings): the families a plain GEMM cannot reach, and the split / persistent
    plans.  The stem, pair and thin-tail kernels are asserted by name in their own tests below."""
    names = set()
    for case in (GENERIC[0], GENERIC[2], POINTWISE[1], POINTWISE[2]):  # K = 72 (one depth block), 270 (two: the folding and split-K forms), 64, 32
        cc = ConvCase(ctx, case)
        for variant in (-1, 0, 3, 4, 8, 11, 20, 24, 27, 28, 30):
            for split in CONV_SPLITS + [(6, 2)]:
                with knobs(ctx, variant, split):
                    names |= kernels_of(ctx, lambda: cc.run(what=f"variant {variant} split {split}"))
    families = {re.match(r"[a-z0-9_]+", nm).group(0) for nm in names}
    print(sorted(names))
    want = {"igemm_f32_kernel", "igemm_f32_dma_kernel", "igemm_f32_dma16_kernel", "igemm_f32_ws_kernel", "igemm_f32_wave_kernel", "igemm_f32_patch_kernel",
            "igemm_f32_pers_kernel", "igemm_f32_lean_kernel"}
    assert families >= want, (sorted(want - families), sorted(names))
    # split-K producers (MODE 2: the last-arrival fold wrote those tiles) of the LDS-DMA, wave and patch families ran on the K = 270 case
    for pattern in (r"igemm_f32_dma_kernel<\d+,\d+,\d+,\d+,2,\d>", r"igemm_f32_wave_kernel<\d+,2,\d+>", r"igemm_f32_patch_kernel<2>"):
        assert any(re.fullmatch(pattern, nm) for nm in names), (pattern, sorted(names))


@pytest.mark.parametrize("c", [8, 30])
def test_conv_thin_tail_tiles(ctx, c):
    """Split mode 4 sends the whole rounds of num_cus tiles to the variant's tile shape and the remaining columns to 16 x 64 tiles.  It needs more tiles
    than compute units: the image width is derived from their number (256 on an MI355X: 70 channels x 2 images of 64 x 65 is 2 x 130 tiles of 64 x 64),
    so the columns past the whole round (and their ragged rows 64..69) are thin tiles.  K = 72: one depth block; K = 270: two."""
    cus = ctx.device_info()["compute_units"]
    w = (cus // 2) // 2 + 1  # 2 images x 64 rows x w columns: tiles_n = 2 * w > cus / 2, so 2 * tiles_n 64 x 64 tiles is one whole round of cus tiles and a tail
    cc = ConvCase(ctx, (2, c, 64, w, 70, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 1))
    for variant in (3, 27):
        with knobs(ctx, variant, (4, 1)):
            names = kernels_of(ctx, lambda: cc.run(what=f"thin tail variant {variant}"))
            assert any(nm.startswith("igemm_f32_thin_kernel") for nm in names), sorted(names)
            cc.run(fused=True, y_lead=1, res_lead=3, what=f"thin tail variant {variant}")


@pytest.mark.parametrize("c", [5, 6])
def test_conv_patch_form(ctx, c):
    """Variant 30: 3x3 / stride 1 / padding 1 with B staged as image patches; w = 10 leaves ragged patch rows, a k-tile is two channels (odd c: a half tile)."""
    cc = ConvCase(ctx, (2, c, 11, 10, 70, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 1))
    for split in ((3, 1), (0, 1), (2, 2)):
        with knobs(ctx, 30, split):
            names = kernels_of(ctx, lambda: cc.run(what=f"patch split {split}"))
            assert any(nm.startswith("igemm_f32_patch_kernel") for nm in names), sorted(names)
            cc.run(fused=True, y_lead=1, res_lead=3, what=f"patch split {split}")
            cc.run(fused=True, y_lead=3, res_lead=1, what=f"patch split {split}")


@pytest.mark.parametrize("o", [24, 64, 70])
def test_conv_stem_form(ctx, o):
    """3-channel 7x7 stride 2 pad 3 on a 37 x 41 image (output 19 x 21: ragged over the 16 x 16 output blocks).  o <= 64 with prepacked weights
    and no residual is the direct stem kernel (variant 32, also the automatic choice), o = 70 the generic gather kernels."""
    cc = ConvCase(ctx, (2, 3, 37, 41, o, 7, 7, (3, 3, 3, 3), (2, 2), (1, 1), 1))
    for variant in (-1, 32, 3):
        with knobs(ctx, variant):
            names = kernels_of(ctx, lambda: cc.run(what=f"stem variant {variant}"))
            stem = any(nm.startswith("conv_small_c_f32_kernel") for nm in names)
            assert stem == (o <= 64 and variant != 3) and (stem or any(nm.startswith("igemm_f32") for nm in names)), (variant, sorted(names))
            for lead in (1, 3):
                cc.run(y_lead=lead, what=f"stem variant {variant}")
            cc.run(act=L.ACT_RELU, want=ref.relu(cc.plain), y_lead=1, what=f"stem variant {variant} relu")
            cc.run(fused=True, y_lead=3, res_lead=1, what=f"stem variant {variant} (a residual takes the generic form)")


def test_conv_grouped(ctx):
    cc = ConvCase(ctx, (2, 8, 11, 13, 6, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 2))
    for variant in VARIANTS:
        with knobs(ctx, variant):
            cc.both(f"grouped variant {variant}")
    for split in CONV_SPLITS:
        with knobs(ctx, 3, split):
            cc.both(f"grouped split {split}")


@pytest.mark.parametrize("h, w", [(5, 8), (6, 8), (5, 12), (6, 12), (5, 10), (6, 10)])
def test_conv_depthwise(ctx, h, w):
    """c = 5 planes.  w % 4 == 0 with aligned pointers is the streaming form (four rows per lane: out_h = 5, 6 are not multiples of 4); off the
    boundary, or w = 10, the `y4` form (out_h >= 4); stride 2 on h = 5 (out_h = 3) the generic one."""
    for stride in (1, 2):
        cc = ConvCase(ctx, (2, 5, h, w, 5, 3, 3, (1, 1, 1, 1), (stride, stride), (1, 1), 5))
        names = kernels_of(ctx, lambda: cc.run(what="depthwise"))
        assert names == {"depthwise_conv2d_f32"}, sorted(names)
        cc.run(fused=True, what="depthwise aligned")
        cc.run(packed=False, what="depthwise OIHW weights")
        cc.both("depthwise")
        cc.run(fused=True, y_lead=3, res_lead=1, what="depthwise")
    cc = ConvCase(ctx, (2, 5, h, w, 5, 5, 5, (2, 2, 2, 2), (1, 1), (1, 1), 5))
    cc.both("depthwise 5x5")


def pointwise_desc(n, c, hw, o):
    return L.Conv2dDesc(n, c, hw, hw, o, 1, 1, (C.c_int32 * 4)(0, 0, 0, 0), 1, 1, 1, 1, 1, hw, hw)


def packed_weights(ctx, d, w):
    w_g = guarded_in(ctx, w)
    p_g = K.Guarded(ctx, ctx.lib.rten_hip_conv2d_f32_packed_bytes(C.byref(d)))
    ctx.call("rten_hip_conv2d_f32_prepack", C.byref(d), w_g.vp, p_g.vp)
    return p_g


def test_conv_pairs(ctx):
    """rten_hip_conv2d_f32_pair / _pair_shortcut on every (M1, M2) their _supported functions accept: n = 1, 9 x 9 -> the forms need
    out_h * out_w % 4 == 0, so 10 x 10 = 100 pixels (ragged over 64) stands in for the 81 of a 9 x 9 image, which they refuse.  Both outputs guarded."""
    n, hw = 1, 10
    assert not ctx.lib.rten_hip_conv2d_f32_pair_supported(C.byref(pointwise_desc(1, 64, 9, 64)), C.byref(pointwise_desc(1, 64, 9, 64)))
    x = K.seeded((n, 64, hw, hw), 1)
    xd = K.seeded((n, 64, hw, hw), 2)
    pairs = shortcuts = 0
    for m1 in (64, 128, 192, 256, 320):
        for m2 in (64, 128, 256):
            d1, d2, ds = pointwise_desc(n, 64, hw, m1), pointwise_desc(n, m1, hw, m2), pointwise_desc(n, 64, hw, m1)
            ok = ctx.lib.rten_hip_conv2d_f32_pair_supported(C.byref(d1), C.byref(d2))
            ok_s = ctx.lib.rten_hip_conv2d_f32_pair_shortcut_supported(C.byref(d1), C.byref(ds), C.byref(d2))
            if not ok and not ok_s:
                continue
            w1, w2, wd = K.seeded((m1, 64, 1, 1), 3, 0.5), K.seeded((m2, m1, 1, 1), 4, 0.25), K.seeded((m1, 64, 1, 1), 5, 0.5)
            b1, b2, bd = K.seeded((m1,), 6), K.seeded((m2,), 7), K.seeded((m1,), 8)
            res = K.seeded((n, m1, hw, hw), 9)
            x_g, xd_g, res_g = guarded_in(ctx, x), guarded_in(ctx, xd), guarded_in(ctx, res)
            p1, p2, pd = packed_weights(ctx, d1, w1), packed_weights(ctx, d2, w2), packed_weights(ctx, ds, wd)
            b1_g, b2_g, bd_g = guarded_in(ctx, b1), guarded_in(ctx, b2), guarded_in(ctx, bd)
            s1, s2 = (n, m1, hw, hw), (n, m2, hw, hw)
            guard = K.nchw_guard(hw * hw)
            for shortcut in (False, True):
                if not (ok_s if shortcut else ok):
                    continue
                y1_g = K.Guarded(ctx, 4 * int(np.prod(s1)), front=guard, back=guard)
                y2_g = K.Guarded(ctx, 4 * int(np.prod(s2)), front=guard, back=guard)
                if shortcut:
                    shortcuts += 1
                    r = ref.conv2d_f32(xd, wd, bd)
                    names = kernels_of(ctx, lambda: ctx.call("rten_hip_conv2d_f32_pair_shortcut", C.byref(d1), x_g.vp, p1.vp, b1_g.vp, C.byref(ds), xd_g.vp, pd.vp, bd_g.vp,
                                                             L.CONV_RELU, y1_g.vp, C.byref(d2), p2.vp, b2_g.vp, L.CONV_RELU, y2_g.vp))
                    assert names == {"conv_pair_f32_kernel<shortcut>"}, sorted(names)
                else:
                    pairs += 1
                    r = res
                    names = kernels_of(ctx, lambda: ctx.call("rten_hip_conv2d_f32_pair", C.byref(d1), x_g.vp, p1.vp, b1_g.vp, res_g.vp, L.CONV_RELU | L.CONV_RESIDUAL,
                                                             y1_g.vp, C.byref(d2), p2.vp, b2_g.vp, L.CONV_RELU, y2_g.vp))
                    assert names == {"conv_pair_f32_kernel"}, sorted(names)
                ctx.sync()
                want1 = ref.conv2d_f32(x, w1, b1, residual=r, relu=True)
                want2 = ref.conv2d_f32(want1, w2, b2, relu=True)
                what = f"pair {m1} -> {m2} shortcut {shortcut}"
                K.bits_equal(y1_g.check(y1_g.raw(), s1, K.dense(s1), F, what + " y1"), want1, what + " y1")
                K.bits_equal(y2_g.check(y2_g.raw(), s2, K.dense(s2), F, what + " y2"), want2, what + " y2")
    assert pairs == 8 and shortcuts == 4, (pairs, shortcuts)  # M1 in {64, 128, 192, 256} x M2 in {64, 128}; the shortcut form: M2 = 64


# ------------------------------------------------------------------------------------------------ convolution: non-finite inputs
@pytest.mark.parametrize("variant", VARIANTS)
def test_conv_nan_image_and_inf_pixels_stay_in_their_windows(ctx, variant):
    """Image 1 all NaN, +Inf at the very last input element (its successor in memory is the guard), -Inf at pixel (0, 0) of image 0: the oracle's
    result -- non-finite exactly on the windows that hold them (tests/test_confine.py) -- on every variant and under a split plan."""
    for name in ("generic-k72", "generic-k270-s2", "pointwise", "grouped"):
        cc = ConvCase(ctx, K.CONV_NONFINITE_CASES[name], nonfinite=True)
        for split in ((3, 1), (2, 3)):
            with knobs(ctx, variant, split):
                cc.run(y_lead=1, what=f"non-finite {name} variant {variant} split {split}")
        with knobs(ctx, variant):
            cc.run(packed=False, what=f"non-finite {name} variant {variant} OIHW")


@pytest.mark.parametrize("name", ["stem", "depthwise"])
def test_conv_nan_image_in_the_direct_kernels(ctx, name):
    cc = ConvCase(ctx, K.CONV_NONFINITE_CASES[name], nonfinite=True)
    for lead in (0, 1):
        cc.run(y_lead=lead, what=f"non-finite {name}")
    if name == "depthwise":
        cc = ConvCase(ctx, (2, 5, 6, 8, 5, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 5), nonfinite=True)  # the streaming form
        cc.run(what="non-finite depthwise streaming")


@pytest.mark.parametrize("c", [5, 6])
def test_conv_nan_image_in_the_patch_form(ctx, c):
    cc = ConvCase(ctx, (2, c, 11, 10, 70, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 1), nonfinite=True)
    for split in ((3, 1), (2, 2)):
        with knobs(ctx, 30, split):
            cc.run(what=f"non-finite patch split {split}")


# ================================================================================================ attention
SDPA_T = [1, 7, 128, 129, 200]


@functools.lru_cache(maxsize=None)
def sdpa_data(s, t, d, mask_kind, nonfinite=False, flush=True):
    q, k, v = K.sdpa_operands(2, 2, s, t, d)
    if nonfinite:
        k = K.sdpa_nonfinite(k)
    mask = None
    if mask_kind == "row":  # [B, 1, 1, T]: batch 0's trailing keys are padding (-inf), the production case
        mask = K.sdpa_trailing_mask(2, t, t // 2)
    elif mask_kind == "full":  # [B, 1, S, T]
        mask = K.seeded((2, 1, s, t), 5, 4.0)
    scale = float(F(1.0) / np.sqrt(F(d)))
    return q, k, v, mask, scale, ref.sdpa(q, k, v, mask=mask, scale=scale, flush_nan=flush)


def run_sdpa(ctx, s, t, d, layout, o_pad, mask_kind, path, nonfinite=False, flush=True):
    B, H = 2, 2
    q, k, v, mask, scale, want = sdpa_data(s, t, d, mask_kind, nonfinite, flush)
    if layout == "bhsd":
        put = lambda a: a
        st = lambda rows: (H * rows * d, rows * d, d)
        o_rs = d + o_pad
        o_st = (H * s * o_rs, s * o_rs, o_rs)
    else:  # [B, S, H, D]: heads interleaved inside a row
        put = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1, 3))
        st = lambda rows: (rows * H * d, d, H * d)
        o_rs = H * d + o_pad
        o_st = (s * o_rs, d, o_rs)
    q_g, k_g, v_g = (guarded_in(ctx, put(a)) for a in (q, k, v))
    m_g = None if mask is None else guarded_in(ctx, mask)
    mbs, mrs = (0, 0) if mask is None else ((t, 0) if mask.shape[2] == 1 and mask_kind == "row" else (s * t, t))
    shape, strides = (B, H, s, d), (*o_st, 1)
    out = K.Guarded(ctx, 4 * K.span(shape, strides), front=K.gemm_guard(o_rs), back=K.gemm_guard(o_rs))
    desc = L.SdpaDesc(B, H, s, t, d, d, *st(s), *st(t), *st(t), *o_st, mbs, mrs, scale, 1 if flush else 0)
    ctx.call("rten_hip_set_sdpa_path", path)
    try:
        ctx.call("rten_hip_sdpa_f32", C.byref(desc), q_g.vp, k_g.vp, v_g.vp, None if m_g is None else m_g.vp, out.vp)
        ctx.sync()
    finally:
        ctx.call("rten_hip_set_sdpa_path", 0)
    what = f"sdpa s {s} t {t} d {d} {layout} o_rs +{o_pad} mask {mask_kind} path {path} non-finite {nonfinite} flush {flush}"
    K.bits_equal(out.check(out.raw(), shape, strides, F, what, ("batch", "head", "row", "column")), want, what)


@pytest.mark.parametrize("t", SDPA_T)
@pytest.mark.parametrize("s", [1, 5, 16, 33, 64])
@pytest.mark.parametrize("d", [32, 64])
def test_sdpa_writes_its_rows_only(ctx, d, s, t):
    """Output rows padded by 4 (keeps the 16-query kernel's `% 4` condition) and by 1 (takes it off) in both layouts, every mask form and path
    (54 launches per item)."""
    for layout in ("bhsd", "bshd"):
        for o_pad in (0, 4, 1):
            for mask_kind in (None, "row", "full"):
                for path in (0, 1, 2):
                    run_sdpa(ctx, s, t, d, layout, o_pad, mask_kind, path)


def test_sdpa_kernels_reached(ctx):
    names = set()
    for (s, t, d) in ((64, 128, 64), (16, 128, 64), (33, 129, 32), (64, 200, 64), (5, 7, 32)):  # the first: the 16-query form (s % 64 == 0, 128 keys, head 64)
        for path in (0, 1, 2):
            names |= kernels_of(ctx, lambda: run_sdpa(ctx, s, t, d, "bshd", 4, "row", path))
            names |= kernels_of(ctx, lambda: run_sdpa(ctx, s, t, d, "bhsd", 1, None, path))
    assert names >= {"sdpa_fused16_kernel", "sdpa_fused_kernel", "sdpa_fused_general_kernel", "softmax_f32"}, sorted(names)


@pytest.mark.parametrize("s, t, d", [(5, 7, 32), (33, 129, 64), (16, 128, 64)])
def test_sdpa_nan_key_stays_in_its_head(ctx, s, t, d):
    """K of (batch 1, head 0) holds a NaN row: out[1, 0] is what the oracle says (zeros with the flush, NaN without), every other head keeps its bits;
    with the [B, 1, 1, T] mask batch 0 has -inf on its trailing keys."""
    for flush in (True, False):
        for mask_kind in (None, "row"):
            for layout in ("bhsd", "bshd"):
                for path in (0, 1, 2):
                    run_sdpa(ctx, s, t, d, layout, 1, mask_kind, path, nonfinite=True, flush=flush)


# ================================================================================================ pooling
def run_pool(ctx, fn, x, kernel, strides, pads, ceil=False, include_pad=False, lead=0, stats=False, want=None):
    n, c, h, w = x.shape
    oh, ow, fp = ref.calc_output_size_and_padding((h, w), kernel, strides, pads, (1, 1), ceil)
    d = L.Pool2dDesc(n, c, h, w, kernel[0], kernel[1], strides[0], strides[1], (C.c_int32 * 4)(*fp), oh, ow, 1 if include_pad else 0)
    if want is None:
        want = ref.max_pool(x, kernel, strides, pads, ceil) if "max" in fn else ref.average_pool(x, kernel, strides, pads, include_pad, ceil)
    x_g = guarded_in(ctx, x, lead)
    guard = K.nchw_guard(oh * ow)
    out = K.Guarded(ctx, want.nbytes, lead=lead, front=guard, back=guard)
    what = f"{fn} {x.shape} k {kernel} s {strides} p {pads} ceil {ceil} lead {lead}"
    if stats:
        nb = ctx.lib.rten_hip_minmax_stats_bytes()
        st = K.Guarded(ctx, nb, itemsize=1)
        ctx.call("rten_hip_minmax_stats_reset", st.vp, 1)
        ctx.call(fn, C.byref(d), x_g.vp, out.vp, st.vp)
        ctx.sync()
        st.check(st.raw(), (nb,), (1,), np.uint8, what + " stats")
    else:
        ctx.call(fn, C.byref(d), x_g.vp, out.vp)
        ctx.sync()
    K.bits_equal(out.check(out.raw(), want.shape, K.dense(want.shape), F, what), want, what)


POOLS = [((3, 3), (2, 2), (1, 1, 1, 1), False), ((2, 2), (2, 2), (0, 0, 0, 0), False), ((5, 5), (3, 3), (0, 0, 0, 0), True)]


@pytest.mark.parametrize("h, w", [(12, 12), (10, 12), (11, 13)])
def test_pooling_writes_its_planes_only(ctx, h, w):
    """3x3 / 2 pad 1 on 12 x 12 and 10 x 12 is the streaming form's geometry (out_h = 6, 5: not multiples of 4) and its neighbours; ceil_mode leaves a partial last window."""
    x = K.seeded((2, 3, h, w), 8)
    for kernel, strides, pads, ceil in POOLS:
        for lead in (0, 1, 3):
            run_pool(ctx, "rten_hip_max_pool2d_f32", x, kernel, strides, pads, ceil, lead=lead)
            for include_pad in (False, True):
                run_pool(ctx, "rten_hip_average_pool2d_f32", x, kernel, strides, pads, ceil, include_pad, lead=lead)
        run_pool(ctx, "rten_hip_max_pool2d_f32_stats", x, kernel, strides, pads, ceil, stats=True)


@pytest.mark.parametrize("inner", [1, 49, 1025])
def test_global_average_pool_writes_nc_values(ctx, inner):
    for nc_shape in ((1, 3), (2, 5)):
        x = K.seeded((*nc_shape, inner), 9)
        want = ref.global_average_pool(x).reshape(-1)
        for lead in (0, 1, 3):
            x_g, out = guarded_in(ctx, x, lead), K.Guarded(ctx, want.nbytes, lead=lead)
            ctx.call("rten_hip_global_average_pool_f32", x.shape[0] * x.shape[1], inner, x_g.vp, out.vp)
            ctx.sync()
            what = f"global average pool {x.shape} lead {lead}"
            K.bits_equal(out.check(out.raw(), want.shape, (1,), F, what), want, what)


@pytest.mark.parametrize("value", [np.nan, -np.inf, np.inf])
def test_pooling_corner_value_stays_in_its_window(ctx, value):
    x = K.pool_nonfinite(K.seeded((2, 3, 12, 12), 8), value)
    for kernel, strides, pads, ceil in POOLS:
        run_pool(ctx, "rten_hip_max_pool2d_f32", x, kernel, strides, pads, ceil)
        run_pool(ctx, "rten_hip_max_pool2d_f32", x, kernel, strides, pads, ceil, lead=1)
        run_pool(ctx, "rten_hip_average_pool2d_f32", x, kernel, strides, pads, ceil)


# ================================================================================================ row-wise kernels
ROWS = [1, 3, 5]
COLS = [1, 3, 16, 17, 255, 256, 257, 1024, 1025, 3000]


def run_rows(ctx, name, x, want, call, lead=0, in_place=False):
    """`call(x_vp, y_vp)` launches the entry point; x and y sit `lead` elements past a 16-byte boundary."""
    x_g = guarded_in(ctx, x, lead)
    out = x_g if in_place else K.Guarded(ctx, want.nbytes, lead=lead)
    call(x_g.vp, out.vp)
    ctx.sync()
    what = f"{name} {x.shape} lead {lead} in place {in_place}"
    K.bits_equal(out.check(out.raw(), want.shape, K.dense(want.shape), F, what), want, what)


def row_ops(ctx, x, rng_seed=0):
    """(name, expected, launcher) for the four row-wise entry points on `x` [rows, cols]."""
    rows, cols = x.shape
    g, b, add = K.seeded((cols,), 4 + rng_seed), K.seeded((cols,), 5 + rng_seed), K.seeded(x.shape, 6 + rng_seed)
    mask = K.seeded((1, cols), 7 + rng_seed, 4.0)
    g_g, b_g, add_g, mask_g = (guarded_in(ctx, a) for a in (g, b, add, mask))
    keep = (g_g, b_g, add_g, mask_g)
    with np.errstate(all="ignore"):
        return [
            ("softmax", ref.softmax(x), lambda xv, yv: ctx.call("rten_hip_softmax_f32", rows, cols, xv, None, 1, 1, 0, yv), keep),
            ("softmax+addend", ref.softmax(x, addend=mask, add_div=rows, add_mod=1),
             lambda xv, yv: ctx.call("rten_hip_softmax_f32", rows, cols, xv, mask_g.vp, rows, 1, 0, yv), keep),
            ("layer_norm", ref.layer_norm(x, g, b), lambda xv, yv: ctx.call("rten_hip_layer_norm_f32", rows, cols, xv, g_g.vp, b_g.vp, 1.0, 0.0, 1e-5, yv), keep),
            ("add_layer_norm", ref.layer_norm(ref.add(x, add), g, b),
             lambda xv, yv: ctx.call("rten_hip_add_layer_norm_f32", rows, cols, xv, add_g.vp, g_g.vp, b_g.vp, 1.0, 0.0, 1e-5, yv), keep),
            ("log_softmax", NR.log_softmax(x), lambda xv, yv: ctx.call("rten_hip_log_softmax_f32", rows, cols, xv, yv), keep),
        ]


@pytest.mark.parametrize("cols", COLS)
def test_row_wise_kernels_write_their_rows_only(ctx, cols):
    for rows in ROWS:
        x = K.seeded((rows, cols), 3, 4.0)
        for name, want, call, _keep in row_ops(ctx, x):
            for lead in (0, 1, 3):
                run_rows(ctx, name, x, want, call, lead)
            run_rows(ctx, name, x, want, call, 1, in_place=True)


def test_layer_norm_streaming_form(ctx):
    """layer_norm_stream_kernel (four rows in sequence per wave) runs from 4 * 4 * 4 * num_cus rows upwards for 128 < cols <= 1024: the smallest such
    launch, with a row count that leaves the last wave a single row, and the smallest cols."""
    rows, cols = 64 * ctx.device_info()["compute_units"] + 1, 129
    x = K.seeded((rows, cols), 3, 4.0)
    g, b, add = K.seeded((cols,), 4), K.seeded((cols,), 5), K.seeded(x.shape, 6)
    g_g, b_g, add_g = guarded_in(ctx, g), guarded_in(ctx, b), guarded_in(ctx, add)
    run_rows(ctx, "layer_norm (streaming)", x, ref.layer_norm(x, g, b), lambda xv, yv: ctx.call("rten_hip_layer_norm_f32", rows, cols, xv, g_g.vp, b_g.vp, 1.0, 0.0, 1e-5, yv), 1)
    run_rows(ctx, "add_layer_norm (streaming)", x, ref.layer_norm(ref.add(x, add), g, b),
             lambda xv, yv: ctx.call("rten_hip_add_layer_norm_f32", rows, cols, xv, add_g.vp, g_g.vp, b_g.vp, 1.0, 0.0, 1e-5, yv), 0, in_place=True)


@pytest.mark.parametrize("cols", K.ROWS_NONFINITE_COLS)
def test_row_wise_non_finite_rows_keep_to_themselves(ctx, cols):
    x, _rows = K.rows_nonfinite(K.seeded((5, cols), 3, 4.0))
    for name, want, call, _keep in row_ops(ctx, x):
        for lead in (0, 1):
            run_rows(ctx, name, x, want, call, lead)


@pytest.mark.parametrize("inner", [1, 1023, 1024, 1025, 4099])
def test_instance_norm_paths(ctx, inner):
    """n * c = 3 slices; automatic, streaming and resident forms; y == x and y != x."""
    x = K.seeded((1, 3, inner), 11, 4.0)
    sc, bi = K.seeded((3,), 12), K.seeded((3,), 13)
    want = NR.instance_norm(x, sc, bi)
    sc_g, bi_g = guarded_in(ctx, sc), guarded_in(ctx, bi)
    for path in (L.INSTANCE_NORM_PATH_AUTO, L.INSTANCE_NORM_PATH_STREAMING, L.INSTANCE_NORM_PATH_RESIDENT):
        ctx.call("rten_hip_set_instance_norm_path", path)
        try:
            call = lambda xv, yv: ctx.call("rten_hip_instance_norm_f32", 1, 3, inner, xv, sc_g.vp, bi_g.vp, 1e-5, L.ACT_NONE, 0.0, 0.0, yv)
            for lead in (0, 1, 3):
                run_rows(ctx, f"instance_norm path {path}", x, want, call, lead)
                run_rows(ctx, f"instance_norm path {path}", x, want, call, lead, in_place=True)
        finally:
            ctx.call("rten_hip_set_instance_norm_path", L.INSTANCE_NORM_PATH_AUTO)


@pytest.mark.parametrize("inner", [1, 5, 49, 1027])
def test_batch_norm_act(ctx, inner):
    x = K.seeded((2, 3, inner), 14, 4.0)
    ps = [K.seeded((3,), 15 + i) for i in range(3)] + [K.seeded((3,), 18) + F(1.0)]
    gs = [guarded_in(ctx, p) for p in ps]
    for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_SIGMOID):
        want = NR.activation(act, NR.batch_norm(x, *ps))
        call = lambda xv, yv: ctx.call("rten_hip_batch_norm_f32_act", 2, 3, inner, xv, gs[0].vp, gs[1].vp, gs[2].vp, gs[3].vp, 1e-5, act, 0.0, 0.0, yv)
        for lead in (0, 1, 3):
            run_rows(ctx, f"batch_norm act {act}", x, want, call, lead)


# ================================================================================================ flat element-wise kernels
FLAT_N = [1, 3, 4, 5, 255, 1023, 1027]
GRID_CAP_N = 2048 * 256 * 4 + 5  # the element-wise grid cap (2048 workgroups of 256 lanes x 4 elements) and an odd tail: the grid-stride loop's second trip
OFFSETS = [(0, 0), (1, 1), (1, 2), (3, 0)]


def run_flat(ctx, what, ins, want, call, x_lead=0, y_lead=0):
    """`ins`: arrays uploaded `x_lead` elements off a 16-byte boundary; `call(*input pointers, y pointer)`."""
    gs = [guarded_in(ctx, a, x_lead) for a in ins]
    out = K.Guarded(ctx, want.nbytes, lead=y_lead, itemsize=want.dtype.itemsize)
    call(*[g.vp for g in gs], out.vp)
    ctx.sync()
    what = f"{what} n {want.size} x+{x_lead} y+{y_lead}"
    K.bits_equal(out.check(out.raw(), want.shape, K.dense(want.shape), want.dtype, what), want, what)


def unary_cases(ctx, n):
    x = K.seeded((n,), 21, 6.0)
    return [("relu", ref.relu(x), lambda xv, yv: ctx.call("rten_hip_relu_f32", n, xv, yv)),
            ("gelu", ref.gelu(x), lambda xv, yv: ctx.call("rten_hip_gelu_f32", n, xv, yv)),
            ("erf", ref.erf(x), lambda xv, yv: ctx.call("rten_hip_erf_f32", n, xv, yv)),
            ("tanh", ref.tanh(x), lambda xv, yv: ctx.call("rten_hip_tanh_f32", n, xv, yv)),
            ("activation sigmoid", NR.activation(L.ACT_SIGMOID, x), lambda xv, yv: ctx.call("rten_hip_activation_f32", L.ACT_SIGMOID, 0.0, 0.0, n, xv, yv))], x


@pytest.mark.parametrize("n", FLAT_N + [GRID_CAP_N])
def test_flat_unary_kernels(ctx, n):
    cases, x = unary_cases(ctx, n)
    for name, want, call in cases:
        for x_lead, y_lead in OFFSETS:
            run_flat(ctx, name, [x], want, call, x_lead, y_lead)


@pytest.mark.parametrize("n", FLAT_N + [GRID_CAP_N])
def test_flat_binary_kernels(ctx, n):
    """b_len == n and b_len < n (trailing-dims broadcast: b_len divides n where it can, 1 otherwise)."""
    a = K.seeded((n,), 22, 4.0)
    blens = sorted({n, 1, 3 if n % 3 == 0 else 1, 5 if n % 5 == 0 else 1})
    for b_len in blens:
        b = K.seeded((b_len,), 23, 2.0) + F(1.5)
        bb = np.resize(b, n)
        for name, want in (("add", ref.add(a, bb)), ("mul", (a * bb).astype(F)), ("sub", (a - bb).astype(F)), ("div", (a / bb).astype(F))):
            call = lambda av, bv, yv, name=name: ctx.call(f"rten_hip_{name}_f32", n, av, bv, b_len, yv)
            for x_lead, y_lead in OFFSETS:
                run_flat(ctx, f"{name} b_len {b_len}", [a, b], want, call, x_lead, y_lead)


@pytest.mark.parametrize("n", FLAT_N + [GRID_CAP_N])
def test_cast_scale_and_dynamic_quantize(ctx, n):
    acc = (K.seeded((n,), 24) * F(2 ** 20)).astype(np.int32)
    for scale_len in sorted({1, 5 if n % 5 == 0 else 1}):
        sc = K.seeded((scale_len,), 25, 0.01) + F(0.02)
        want = ref.cast_scale(acc.reshape(-1, scale_len), sc if scale_len > 1 else sc.reshape(())).reshape(-1)
        for x_lead, y_lead in OFFSETS:
            run_flat(ctx, f"cast_scale scale_len {scale_len}", [acc, sc], want, lambda xv, sv, yv: ctx.call("rten_hip_cast_scale", n, xv, sv, scale_len, yv), x_lead, y_lead)
    # DynamicQuantizeLinear: a uint8 output (both fills), and two one-element outputs
    x = K.seeded((n,), 26, 6.0)
    q, s, z = ref.dynamic_quantize_linear(x)
    for fill in K.FILLS_8BIT:
        for x_lead, y_lead in OFFSETS:
            x_g = guarded_in(ctx, x, x_lead)
            y_g = K.Guarded(ctx, n, lead=y_lead, fill=fill, itemsize=1)
            s_g, z_g = K.Guarded(ctx, 4), K.Guarded(ctx, 1, fill=fill, itemsize=1)
            ctx.call("rten_hip_dynamic_quantize_linear", n, x_g.vp, y_g.vp, s_g.vp, z_g.vp)
            ctx.sync()
            what = f"dynamic_quantize_linear n {n} fill {fill:#x} x+{x_lead} y+{y_lead}"
            K.bits_equal(y_g.check(y_g.raw(), (n,), (1,), np.uint8, what), q.reshape(-1), what)
            assert s_g.check(s_g.raw(), (1,), (1,), F, what + " scale")[0] == s
            assert z_g.check(z_g.raw(), (1,), (1,), np.uint8, what + " zero point")[0] == z


def test_add_channel_bias_and_copy_rows(ctx):
    for inner in (1, 3, 5, 67):
        x, b = K.seeded((2, 3, inner), 27), K.seeded((3,), 28)
        want = (x + b[None, :, None]).astype(F)
        for x_lead, y_lead in OFFSETS:
            run_flat(ctx, "add_channel_bias", [x], want, lambda xv, yv, b_g=guarded_in(ctx, b): ctx.call("rten_hip_add_channel_bias_f32", 2, 3, inner, xv, b_g.vp, yv), x_lead, y_lead)
    # copy_rows: a Concat piece written into its slot -- destination rows have a gap that must keep the fill
    for row_elems in (1, 3, 5, 67):
        rows, src_pitch, dst_pitch = 5, row_elems + 2, row_elems + 3
        src = K.seeded((rows, src_pitch), 29)
        for lead in (0, 1, 3):
            s_g = guarded_in(ctx, src, lead)
            shape, strides = (rows, row_elems), (dst_pitch, 1)
            out = K.Guarded(ctx, 4 * K.span(shape, strides), lead=lead)
            ctx.call("rten_hip_copy_rows_b32", rows, row_elems, s_g.vp, src_pitch, out.vp, dst_pitch)
            ctx.sync()
            what = f"copy_rows {rows} x {row_elems} lead {lead}"
            K.bits_equal(out.check(out.raw(), shape, strides, F, what), src[:, :row_elems], what)


# ================================================================================================ int8 GEMM
def int8_operands(m, k, n, a_dt, b_dt, batch):
    """Random codes with the extreme codes of each type in the last row, the last column and the last k of both operands: the lanes beside the
    padding.  Zero points are far from 0, so a padding byte taken as the zero CODE (instead of the zero point) would change the sums."""
    rng = ref.XorShiftRng(500 + m + n)
    gen = lambda dt, cnt: (rng.u8(cnt) if dt == np.uint8 else rng.i8(cnt))
    a = gen(a_dt, batch * m * k).reshape(batch, m, k)
    b = gen(b_dt, batch * k * n).reshape(batch, k, n)
    lo_a, hi_a, lo_b, hi_b = np.iinfo(a_dt).min, np.iinfo(a_dt).max, np.iinfo(b_dt).min, np.iinfo(b_dt).max
    a[:, -1, ::2], a[:, -1, 1::2], a[:, ::2, -1], a[:, 1::2, -1] = hi_a, lo_a, lo_a, hi_a
    b[:, -1, ::2], b[:, -1, 1::2], b[:, ::2, -1], b[:, 1::2, -1] = hi_b, lo_b, lo_b, hi_b
    # zero points: never the raw zero code, and never the code that becomes 0 when a u8 operand is shifted into the signed domain (128) or its i8
    # image (-128), so that a padding byte taken as a raw 0 in either domain cannot pass for "operand equals zero point"
    def zero_points(dt, cnt, last):
        z = gen(dt, cnt)
        z[(z == 0) | (z == (128 if dt == np.uint8 else -128))] = 77
        z[-1] = last
        assert not ((z == 0) | (z.astype(np.int32) == 128) | (z.astype(np.int32) == -128)).any()
        return z
    return a, b, zero_points(a_dt, m, hi_a), zero_points(b_dt, n, hi_b)


@pytest.mark.parametrize("a_dt, b_dt", [(np.uint8, np.int8), (np.int8, np.uint8)], ids=["u8i8", "i8u8"])
@pytest.mark.parametrize("m, k, n", [(65, 100, 129), (130, 272, 70)])
def test_gemm_int8_writes_its_rows_only(ctx, m, k, n, a_dt, b_dt):
    """ldc = n + 3 and a c_bs gap, int32 and f32 outputs, both int8 paths, every tile, prepacked (one product) and plain B (batch 2)."""
    ldc = n + 3
    a, b, a_zp, b_zp = int8_operands(m, k, n, a_dt, b_dt, 2)
    acc = np.stack([ref.gemm_int8(a[z], b[z], a_zp, b_zp) for z in range(2)])
    scale = K.seeded((n,), 31, 0.01) + F(0.02)
    want_f = np.stack([ref.cast_scale(acc[z], scale) for z in range(2)])
    a_g, b_g, az_g, bz_g, sc_g = (guarded_in(ctx, v) for v in (a, b, a_zp, b_zp, scale))
    nb = ctx.lib.rten_hip_gemm_int8_packed_bytes(k, n)
    assert nb
    p_g = K.Guarded(ctx, nb, itemsize=1)  # exactly packed_bytes inside guards
    ctx.call("rten_hip_gemm_int8_prepack", k, n, b_g.vp, n, 1, 1 if b_dt == np.int8 else 0, p_g.vp)
    ctx.sync()
    p_g.check(p_g.raw(), (nb,), (1,), np.uint8, f"gemm_int8_prepack {k} x {n}")
    try:
        for path in (0, 1):
            ctx.call("rten_hip_set_int8_path", path)
            for tile in (-1, 0, 1, 2, 3):
                ctx.call("rten_hip_set_int8_tile", tile, None)
                for prepacked in (True, False):
                    batch = 1 if prepacked else 2
                    c_bs = m * ldc + 5
                    shape, strides = (batch, m, n), (c_bs, ldc, 1)
                    for as_f32 in (False, True):
                        for lead in (0, 1):
                            out = K.Guarded(ctx, 4 * K.span(shape, strides), lead=lead, front=K.gemm_guard(ldc), back=K.gemm_guard(ldc))
                            d = L.GemmInt8Desc(m, n, k, k, 1, n, 1, ldc, int(a_dt == np.int8), int(b_dt == np.int8), m, n, n if as_f32 else 0,
                                               batch, m * k, k * n, c_bs, 1 if prepacked else 0)
                            ctx.call("rten_hip_gemm_int8", C.byref(d), a_g.vp, p_g.vp if prepacked else b_g.vp, az_g.vp, bz_g.vp, sc_g.vp if as_f32 else None, out.vp)
                            ctx.sync()
                            what = f"gemm_int8 {m}x{k}x{n} path {path} tile {tile} prepacked {prepacked} f32 {as_f32} lead {lead}"
                            got = out.check(out.raw(), shape, strides, F if as_f32 else np.int32, what)
                            K.bits_equal(got, (want_f if as_f32 else acc)[:batch], what)
    finally:
        ctx.call("rten_hip_set_int8_path", 0)
        ctx.call("rten_hip_set_int8_tile", -1, None)


# ================================================================================================ ConvTranspose
def run_conv_transpose(ctx, cg, og, k, stride, dil=1, groups=1, opad=(0, 0), lead=0, nan_image=False, want_kernel=None):
    n, h, w = 2, 5, 7
    x = K.seeded((n, cg * groups, h, w), 41)
    if nan_image:
        x[1] = np.nan
    wt, b = K.seeded((cg * groups, og, k, k), 42, 0.5), K.seeded((og * groups,), 43)
    pads = (1, 0, 0, 1) if k > 2 else (0, 0, 0, 0)
    want = ref.conv_transpose2d_f32(x, wt, b, pads, (stride, stride), (dil, dil), groups, opad)
    oh, ow = want.shape[2:]
    d = L.Conv2dDesc(n, cg * groups, h, w, og * groups, k, k, (C.c_int32 * 4)(*pads), stride, stride, dil, dil, groups, oh, ow)
    x_g, w_g, b_g = guarded_in(ctx, x), guarded_in(ctx, wt), guarded_in(ctx, b)
    guard = K.nchw_guard(oh * ow)
    out = K.Guarded(ctx, want.nbytes, lead=lead, front=guard, back=guard)
    names = kernels_of(ctx, lambda: ctx.call("rten_hip_conv_transpose2d_f32", C.byref(d), x_g.vp, w_g.vp, b_g.vp, out.vp))
    what = f"conv_transpose C_g {cg} O_g {og} k {k} stride {stride} dil {dil} groups {groups} output_padding {opad} lead {lead} NaN image {nan_image}"
    if want_kernel:
        assert want_kernel in names, (what, sorted(names))
    K.bits_equal(out.check(out.raw(), want.shape, K.dense(want.shape), F, what), want, what)
    if nan_image:
        assert np.isnan(want[1]).any() and np.isfinite(want[0]).all()  # (with a dilated kernel some output pixels of image 1 receive no tap: bias only)


def conv_transpose_form(cg, og, k, stride):
    """The fused kernel keeps ceil(k / stride) * k taps of C_g channels for 16 / 32 / 64 output channels in LDS and runs while that fits 64 KiB
    (conv_transpose.hip); beyond it -- C_g 64 / 68 with O_g = 64 on the 4x4 and 3x3 kernels -- the call is the GEMM + col2im sequence."""
    jt = 1 if og <= 16 else 2 if og <= 32 else 4
    lds = -(-k // stride) * k * cg * 16 * jt * 4
    return "conv_transpose_fused_kernel" if lds <= 64 * 1024 else "col2im_f32"


@pytest.mark.parametrize("cg", [4, 64, 68])
@pytest.mark.parametrize("og", [3, 16, 64])
def test_conv_transpose_fused_form(ctx, cg, og):
    forms = set()
    for k, stride in ((4, 2), (3, 1), (2, 2)):
        form = conv_transpose_form(cg, og, k, stride)
        forms.add(form)
        for opad in ((0, 0), (1, 1)) if stride == 2 else ((0, 0),):
            for lead in (0, 1, 3):
                run_conv_transpose(ctx, cg, og, k, stride, opad=opad, lead=lead, want_kernel=form)
    assert "conv_transpose_fused_kernel" in forms  # (2x2 / stride 2 fits at every size here)
    run_conv_transpose(ctx, cg, og, 2, 2, groups=2, want_kernel="conv_transpose_fused_kernel")
    run_conv_transpose(ctx, cg, og, 2, 2, lead=1, nan_image=True, want_kernel="conv_transpose_fused_kernel")
    run_conv_transpose(ctx, cg, og, 4, 2, lead=1, nan_image=True, want_kernel=conv_transpose_form(cg, og, 4, 2))


def test_conv_transpose_composed_form(ctx):
    """C_g = 5 (no 16-byte channel groups) or dilation 2: the GEMM into a column matrix (ldc = P, c_bs = M * P) + col2im."""
    for cg, dil in ((5, 1), (4, 2), (5, 2)):
        for og in (3, 16):
            for lead in (0, 1, 3):
                run_conv_transpose(ctx, cg, og, 3, 2, dil=dil, opad=(1, 0), lead=lead, want_kernel="col2im_f32")
            run_conv_transpose(ctx, cg, og, 3, 2, dil=dil, groups=2, nan_image=True, want_kernel="col2im_f32")


# ================================================================================================ GRU / LSTM
RNN_DIR = {"forward": L.RNN_FORWARD, "reverse": L.RNN_REVERSE, "bidirectional": L.RNN_BIDIRECTIONAL}


def run_rnn(ctx, lstm, hidden, batch, path, nan_row=None, lead=0):
    from tests import rnn_rules as R
    seq, n_in, direction, dirs, G = 3, 6, "bidirectional", 2, 4 if lstm else 3
    rng = np.random.default_rng(hidden * 100 + batch)
    u = lambda *s, k=1.0: ((rng.random(s, dtype=F) - F(0.5)) * F(2 * k)).astype(F)
    x, w, r = u(seq, batch, n_in), u(dirs, G * hidden, n_in, k=0.4), u(dirs, G * hidden, hidden, k=0.4)
    b, h0, c0 = u(dirs, 2 * G * hidden, k=0.5), u(dirs, batch, hidden), u(dirs, batch, hidden)
    if nan_row is not None:
        x[0, nan_row] = np.nan
    with np.errstate(all="ignore"):
        want = R.lstm(x, w, r, b, h0, c0, direction) if lstm else R.gru(x, w, r, b, h0, direction)
    ins = [guarded_in(ctx, a) for a in ((x, w, r, b, h0, c0) if lstm else (x, w, r, b, h0))]
    shapes = [(seq, dirs, batch, hidden), (dirs, batch, hidden), (dirs, batch, hidden)][:len(want)]
    outs = [K.Guarded(ctx, 4 * int(np.prod(s)), lead=lead) for s in shapes]
    ctx.call("rten_hip_set_rnn_path", path)
    try:
        if lstm:
            ctx.call("rten_hip_lstm_f32", seq, batch, n_in, hidden, RNN_DIR[direction], 0, 0, *[g.vp for g in ins], *[o.vp for o in outs])
        else:
            ctx.call("rten_hip_gru_f32", seq, batch, n_in, hidden, RNN_DIR[direction], 1, 0, 0, *[g.vp for g in ins], *[o.vp for o in outs])
        ctx.sync()
    finally:
        ctx.call("rten_hip_set_rnn_path", L.RNN_PATH_AUTO)
    for name, o, s, wv in zip(("Y", "Y_h", "Y_c"), outs, shapes, want):
        what = f"{'lstm' if lstm else 'gru'} hidden {hidden} batch {batch} path {path} NaN row {nan_row} lead {lead} {name}"
        K.bits_equal(o.check(o.raw(), s, K.dense(s), F, what), wv, what)
    return want


@pytest.mark.parametrize("lstm", [False, True], ids=["gru", "lstm"])
@pytest.mark.parametrize("path", [L.RNN_PATH_COMPOSED, L.RNN_PATH_FUSED], ids=["composed", "fused"])
def test_rnn_outputs_are_written_exactly(ctx, lstm, path):
    """hidden 3 is below an MFMA tile, 20 puts gate boundaries inside one; batch 17 is a 16-row tile plus one row and 15 rows of padding."""
    for hidden in (3, 20):
        for batch in (1, 17):
            if path == L.RNN_PATH_FUSED and batch == 1:
                continue  # one row and fewer than five steps: the reference's vector-matrix order, which the fused kernel does not cover (rten_hip.h)
            for lead in (0, 1):
                run_rnn(ctx, lstm, hidden, batch, path, lead=lead)


@pytest.mark.parametrize("lstm", [False, True], ids=["gru", "lstm"])
@pytest.mark.parametrize("path", [L.RNN_PATH_COMPOSED, L.RNN_PATH_FUSED], ids=["composed", "fused"])
def test_rnn_nan_batch_row_stays_in_its_row(ctx, lstm, path):
    """Batch row 3 of x is NaN at t = 0: with batch 17 it shares a 16-row tile with finite rows.  The restated reference keeps it to batch row 3 of
    every output (asserted here on the expectation); the device must give those bits."""
    for hidden in (3, 20):
        want = run_rnn(ctx, lstm, hidden, 17, path, nan_row=3)
        for o in want:
            bad = ~np.isfinite(o)
            assert bad[..., 3, :].any() and not np.delete(bad, 3, axis=-2).any()


# ================================================================================================ layout, selection and reduction kernels
INNER = [1, 3, 5, 67]


def i64(v):
    return (C.c_int64 * max(len(v), 1))(*v)


def layout_check(ctx, what, ins, want, call, leads=(0, 1, 3), fills=(K.FILL,)):
    """`call(*input pointers, y pointer)` into a guarded y of want's dtype, inputs and y `lead` elements off a 16-byte boundary."""
    for fill in fills:
        for lead in leads:
            gs = [guarded_in(ctx, a, lead) for a in ins]
            out = K.Guarded(ctx, want.nbytes, lead=lead, fill=fill, itemsize=want.dtype.itemsize)
            call(*[g.vp for g in gs], out.vp)
            ctx.sync()
            w = f"{what} lead {lead} fill {fill:#x}"
            K.bits_equal(out.check(out.raw(), want.shape, K.dense(want.shape), want.dtype, w), want, w)


@pytest.mark.parametrize("e", INNER)
def test_layout_kernels_write_their_output_only(ctx, e):
    from rten_amd import ops as O
    x = K.seeded((3, 4, e), 51)
    # transpose: every permutation of a rank-3 tensor whose innermost extent is e
    for perm in ((0, 2, 1), (2, 1, 0), (1, 0, 2), (2, 0, 1), (0, 1, 2)):
        layout_check(ctx, f"transpose {x.shape} {perm}", [x], np.ascontiguousarray(x.transpose(perm)),
                     lambda xv, yv: ctx.call("rten_hip_transpose_b32", 3, i64(x.shape), (C.c_int32 * 3)(*perm), xv, yv))
    # copy_strided: a permuted view, a broadcast axis (stride 0) and a slice of a wider tensor
    for shape, strides in (((e, 4, 3), (1, e, 4 * e)), ((3, 5, e), (4 * e, 0, 1)), ((3, 2, e), (4 * e, 2 * e, 1))):
        want = np.ascontiguousarray(np.lib.stride_tricks.as_strided(x, shape, [4 * s for s in strides]))
        layout_check(ctx, f"copy_strided {shape} {strides}", [x], want, lambda xv, yv: ctx.call("rten_hip_copy_strided_b32", 3, i64(shape), i64(strides), xv, yv))
    # binary_broadcast: [3, 4, e] op [4, 1] and op a single element
    for b in (K.seeded((4, 1), 52) + F(1.5), K.seeded((1,), 53) + F(1.5)):
        bs = (0, 1, 0) if b.size > 1 else (0, 0, 0)
        for op, fn in ((L.BINARY_ADD, np.add), (L.BINARY_DIV, np.divide), (L.BINARY_MAX, np.maximum)):
            layout_check(ctx, f"binary_broadcast op {op} b {b.shape}", [x, b], fn(x, b.reshape(-1, 1) if b.size > 1 else b).astype(F),
                         lambda xv, bv, yv: ctx.call("rten_hip_binary_broadcast_f32", op, 3, i64(x.shape), i64(K.dense(x.shape)), i64(bs), xv, bv, yv))
    # elementwise_nd: int32 add with a broadcast operand
    a32, b32 = (x * 1000).astype(np.int32), np.arange(4, dtype=np.int32).reshape(4, 1) - 2
    layout_check(ctx, "elementwise_nd iadd", [a32, b32], (a32 + b32).astype(np.int32),
                 lambda av, bv, yv: ctx.call("rten_hip_elementwise_nd", L.EW_IADD, 3, i64(x.shape), av, L.DT_I32, i64(K.dense(x.shape)), bv, L.DT_I32, i64((0, 1, 0)), None, None, yv, L.DT_I32))
    # gather along an axis, and rows of a table
    ids = np.array([3, 0, -1, 2, 2], np.int32)
    layout_check(ctx, "gather_axis", [x, ids], np.take(x, ids, axis=1), lambda xv, iv, yv: ctx.call("rten_hip_gather_axis_b32", 3, 4, e, ids.size, xv, iv, yv))
    table, rid = K.seeded((7, e), 54), np.array([6, 0, 3, 3, 1], np.int32)
    layout_check(ctx, "gather_rows", [table, rid], table[rid], lambda tv, iv, yv: ctx.call("rten_hip_gather_rows_f32", rid.size, e, 7, tv, iv, yv))
    del O


@pytest.mark.parametrize("e", INNER)
def test_reductions_and_selection_write_their_output_only(ctx, e):
    from oracle import einsum as OE
    from tests import select_rules as S
    x = K.seeded((3, 5, e), 55, 8.0)
    last = dict(osh=(3, 5), ost=(5 * e, e), ish=(e,), ist=(1,), axes=[2])       # over the innermost axis
    mid = dict(osh=(3, e), ost=(5 * e, 1), ish=(5,), ist=(e,), axes=[1])        # over the middle axis: the output's innermost extent is e
    for g in (last, mid):
        for name, fn in (("rten_hip_reduce_sum_strided_f32", OE.reduce_sum), ("rten_hip_reduce_mean_strided_f32", OE.reduce_mean)):
            layout_check(ctx, f"{name} axes {g['axes']}", [x], fn(x, g["axes"], False),
                         lambda xv, yv: ctx.call(name, 2, i64(g["osh"]), i64(g["ost"]), 1, i64(g["ish"]), i64(g["ist"]), xv, yv))
        for op, opname in ((0, "max"), (1, "min")):
            layout_check(ctx, f"reduce_minmax {opname} axes {g['axes']}", [x], S.reduce_minmax(x, g["axes"], False, opname),
                         lambda xv, yv: ctx.call("rten_hip_reduce_minmax_strided", op, L.DT_F32, 2, i64(g["osh"]), i64(g["ost"]), 1, i64(g["ish"]), i64(g["ist"]), xv, yv))
            layout_check(ctx, f"arg_minmax {opname} axes {g['axes']}", [x], S.arg_minmax(x, g["axes"][0], False, opname),
                         lambda xv, yv: ctx.call("rten_hip_arg_minmax_strided", op, L.DT_F32, 2, i64(g["osh"]), i64(g["ost"]), g["ish"][0], g["ist"][0], xv, yv))
    # TopK along the innermost axis: both outputs guarded
    k = min(2, e)
    vals, idx = S.topk(x, k, -1, True)
    for lead in (0, 1, 3):
        x_g = guarded_in(ctx, x, lead)
        v_g, i_g = K.Guarded(ctx, vals.nbytes, lead=lead), K.Guarded(ctx, idx.nbytes, lead=lead)
        ctx.call("rten_hip_topk_strided", 1, L.DT_F32, 2, i64((3, 5)), i64((5 * e, e)), i64((5 * k, k)), e, 1, k, x_g.vp, v_g.vp, i_g.vp, 1)
        ctx.sync()
        K.bits_equal(v_g.check(v_g.raw(), vals.shape, K.dense(vals.shape), F, "topk values"), vals, f"topk values e {e} lead {lead}")
        K.bits_equal(i_g.check(i_g.raw(), idx.shape, K.dense(idx.shape), np.int32, "topk indices"), idx, f"topk indices e {e} lead {lead}")


@pytest.mark.parametrize("rows", [1, 3])
def test_matmul_nbits(ctx, rows):
    """rows = 1: the 4-bit vector kernel; rows = 3: dequantisation into scratch + the f32 GEMM."""
    for n_cols, n_blocks, bs in ((5, 3, 32), (67, 2, 16), (130, 9, 32)):
        rng = ref.XorShiftRng(60 + n_cols)
        k = n_blocks * bs
        lhs = (rng.f32(rows * k) - F(0.5)).reshape(rows, k)
        quant = rng.u8(n_cols * n_blocks * (bs // 2)).reshape(n_cols, n_blocks, bs // 2)
        scales = rng.f32(n_cols * n_blocks).reshape(n_cols, n_blocks)
        want = ref.matmul_nbits_f32(lhs, quant, scales)
        layout_check(ctx, f"matmul_nbits rows {rows} n {n_cols} k {k}", [lhs], want,
                     lambda lv, yv, q_g=guarded_in(ctx, quant), s_g=guarded_in(ctx, scales): ctx.call("rten_hip_matmul_nbits_f32", 1, rows, k, n_cols, bs, lv, q_g.vp, s_g.vp, yv),
                     leads=(0,) if rows == 1 else (0, 1))


# ================================================================================================ int8 convolution and its staged buffers
INT8_CONVS = [(2, 40, 11, 13, 70, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 1),    # o = 70: a ragged second tile of output channels; c = 40: channels padded to 48
              (2, 3, 21, 23, 70, 7, 7, (3, 3, 3, 3), (2, 2), (1, 1), 1),     # c = 3: the packed few-channel stem form
              (3, 64, 7, 7, 70, 1, 1, (0, 0, 0, 0), (1, 1), (1, 1), 1)]      # pointwise, 147 columns


def int8_conv_operands(case):
    """u8 activations and i8 weights with the extreme codes at the last pixel / channel / tap; the zero point (131) is far from the zero code, so is the
    padding value of PAD_RAW0_* from the zero point."""
    n, c, h, w, o, kh, kw = case[:7]
    rng = ref.XorShiftRng(700 + c)
    x = rng.u8(n * c * h * w).reshape(n, c, h, w)
    wt = rng.i8(o * c * kh * kw, reduced=True).reshape(o, c, kh, kw)
    x[:, -1, -1, ::2], x[:, -1, -1, 1::2], x[-1, :, :, -1] = 255, 0, 255
    wt[-1, :, -1, -1], wt[::2, -1, -1, -1] = wt.max(), wt.min()
    return x, wt


@pytest.mark.parametrize("case", INT8_CONVS, ids=["3x3-c40", "stem-c3", "1x1-c64"])
def test_conv_int8_writes_its_planes_only(ctx, case):
    n, c, h, w, o, kh, kw, pads, strides, dil, groups = case
    d32, oh, ow = conv_desc(case)
    x, wt = int8_conv_operands(case)
    zp, scale, bias = np.array(131, np.uint8), np.array(0.0123, F), K.seeded((o,), 71)
    x_g, w_g, zp_g, sc_g, b_g = (guarded_in(ctx, v) for v in (x, wt, zp.reshape(1), scale.reshape(1), bias))
    shape = (n, o, oh, ow)
    guard = K.nchw_guard(oh * ow)
    try:
        for path in (0, 1):
            ctx.call("rten_hip_set_int8_path", path)
            for pm in (L.PAD_ZERO_POINT, L.PAD_RAW0_I8, L.PAD_RAW0_U8):
                acc = ref.conv2d_int8(x, wt, x_zp=131, pads=pads, strides=strides, pad_mode=pm)
                want_f = ref.relu(ref.cast_scale(acc, scale) + bias[None, :, None, None])
                for as_f32 in (False, True):
                    for lead in (0, 1):
                        d = L.Conv2dInt8Desc(d32, 0, 1, 0, pm, 0, 0, 1 if as_f32 else 0)
                        out = K.Guarded(ctx, 4 * int(np.prod(shape)), lead=lead, front=guard, back=guard)
                        ctx.call("rten_hip_conv2d_int8", C.byref(d), x_g.vp, w_g.vp, zp_g.vp, None, sc_g.vp if as_f32 else None, b_g.vp if as_f32 else None, None,
                                 L.CONV_RELU if as_f32 else 0, out.vp)
                        ctx.sync()
                        what = f"conv2d_int8 {case} path {path} pad_mode {pm} f32 {as_f32} lead {lead}"
                        got = out.check(out.raw(), shape, K.dense(shape), F if as_f32 else np.int32, what)
                        K.bits_equal(got, want_f if as_f32 else acc, what)
    finally:
        ctx.call("rten_hip_set_int8_path", 0)


@pytest.mark.parametrize("case", INT8_CONVS, ids=["3x3-c40", "stem-c3", "1x1-c64"])
def test_conv_int8_staged_buffers_have_exactly_their_stated_size(ctx, case):
    """rten_hip_conv2d_int8_prepack, rten_hip_dynamic_quantize_linear_staged, _staged_stats and _staged_products each write into a buffer of exactly
    rten_hip_conv2d_int8_packed_bytes() / _staged_bytes() inside guards (8-bit data: both fills); the convolution on the staged operands gives the oracle's bits."""
    n, c, h, w, o, kh, kw, pads, strides, dil, groups = case
    d32, oh, ow = conv_desc(case)
    d = L.Conv2dInt8Desc(d32, 0, 1, 0, L.PAD_RAW0_I8, 1, 1, 1)
    _, wt = int8_conv_operands(case)
    # the float input is a MaxPool's output, so that the pool's statistics block can feed the _stats form
    x0 = K.seeded((n, c, 2 * h, 2 * w), 72, 6.0)
    x = ref.max_pool(x0, (2, 2), (2, 2))
    q, s, z = ref.dynamic_quantize_linear(x)
    w_scale = np.array([0.003, 0.007], F)
    acc = ref.conv2d_int8(q, wt, x_zp=int(z), pads=pads, strides=strides, pad_mode=ref.PAD_RAW0_I8)
    shape = (n, o, oh, ow)
    pool_d = L.Pool2dDesc(n, c, 2 * h, 2 * w, 2, 2, 2, 2, (C.c_int32 * 4)(0, 0, 0, 0), h, w, 0)
    x0_g, w_g, ws_g = guarded_in(ctx, x0), guarded_in(ctx, wt), guarded_in(ctx, w_scale)
    ws1_vp = C.c_void_p(ws_g.ptr + 4)
    nb_p, nb_s, nb_st = (ctx.lib.rten_hip_conv2d_int8_packed_bytes(C.byref(d)), ctx.lib.rten_hip_conv2d_int8_staged_bytes(C.byref(d)), ctx.lib.rten_hip_minmax_stats_bytes())
    assert nb_p and nb_s
    for fill in K.FILLS_8BIT:
        packed = K.Guarded(ctx, nb_p, fill=fill, itemsize=1)
        ctx.call("rten_hip_conv2d_int8_prepack", C.byref(d), w_g.vp, packed.vp)
        stats = K.Guarded(ctx, nb_st, fill=fill, itemsize=1)
        ctx.call("rten_hip_minmax_stats_reset", stats.vp, 1)
        x_g = K.Guarded(ctx, x.nbytes)
        ctx.call("rten_hip_max_pool2d_f32_stats", C.byref(pool_d), x0_g.vp, x_g.vp, stats.vp)
        ctx.sync()
        packed.check(packed.raw(), (nb_p,), (1,), np.uint8, f"conv2d_int8_prepack fill {fill:#x}")
        stats.check(stats.raw(), (nb_st,), (1,), np.uint8, f"minmax stats fill {fill:#x}")
        K.bits_equal(x_g.check(x_g.raw(), x.shape, K.dense(x.shape), F, "max_pool_stats"), x, "max_pool_stats")
        for form in ("staged", "stats", "products"):
            staged = K.Guarded(ctx, nb_s, fill=fill, itemsize=1)
            xs, xz = K.Guarded(ctx, 4), K.Guarded(ctx, 1, fill=fill, itemsize=1)
            prods = [K.Guarded(ctx, 4), K.Guarded(ctx, 4)]
            if form == "staged":
                ctx.call("rten_hip_dynamic_quantize_linear_staged", C.byref(d), x_g.vp, staged.vp, xs.vp, xz.vp, ws_g.vp, prods[0].vp)
            elif form == "stats":
                ctx.call("rten_hip_dynamic_quantize_linear_staged_stats", C.byref(d), x_g.vp, stats.vp, staged.vp, xs.vp, xz.vp, ws_g.vp, prods[0].vp)
            else:
                mul_by, product = (C.c_void_p * 2)(ws_g.vp, ws1_vp), (C.c_void_p * 2)(prods[0].vp, prods[1].vp)
                ctx.call("rten_hip_dynamic_quantize_linear_staged_products", C.byref(d), x_g.vp, None, staged.vp, xs.vp, xz.vp, 2, mul_by, product)
            ctx.sync()
            what = f"dynamic_quantize_linear_{form} {case} fill {fill:#x}"
            staged.check(staged.raw(), (nb_s,), (1,), np.uint8, what + " staged image")
            assert xs.check(xs.raw(), (1,), (1,), F, what + " scale")[0] == s and xz.check(xz.raw(), (1,), (1,), np.uint8, what + " zero point")[0] == z
            for i in range(2 if form == "products" else 1):
                assert prods[i].check(prods[i].raw(), (1,), (1,), F, what + " product")[0] == F(F(s) * w_scale[i])
            # the convolution reads the staged image and the packed weights: int32 and f32 outputs
            guard = K.nchw_guard(oh * ow)
            for as_f32 in (False, True):
                dd = L.Conv2dInt8Desc(d32, 0, 1, 0, L.PAD_RAW0_I8, 1, 1, 1 if as_f32 else 0)
                out = K.Guarded(ctx, 4 * int(np.prod(shape)), lead=1, front=guard, back=guard)
                ctx.call("rten_hip_conv2d_int8", C.byref(dd), staged.vp, packed.vp, xz.vp, None, prods[0].vp if as_f32 else None, None, None, 0, out.vp)
                ctx.sync()
                got = out.check(out.raw(), shape, K.dense(shape), F if as_f32 else np.int32, what + " conv")
                K.bits_equal(got, ref.cast_scale(acc, F(F(s) * w_scale[0])) if as_f32 else acc, what + " conv")
