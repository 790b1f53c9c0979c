"""MatMulNBits with more than one row on the fused kernel (rten_amd/csrc/matmul_nbits_gemm.hip, rten_hip_set_nbits_path 2): bit for bit against the oracle at
every tile edge, between guards (tests/confine.py) on both tiles and with non-finite rows and columns, inside the forward error bound of an f32 FMA chain
against float64, on scales whose eightfold overflows, on every mode of the setter, and captured into a hipGraph on a context that never ran the shape eagerly."""
import functools

import numpy as np
import pytest

from oracle import ref
from rten_amd import lib as L
from rten_amd.tensor import DeviceTensor
from tests import attention_cases as AC
from tests import confine as K
from tests import range_cases as RC
from tests.reduce_rules import same_bits

F = np.float32
pytestmark = pytest.mark.gpu
AUTO, EXPAND, FUSED = 0, 1, 2  # rten_hip_set_nbits_path


draw = AC.nbits_operands  # lhs [*lead, k] in [-0.5, 0.5), every code, scales in [0, 1), as tests/test_gpu_parity.py::test_matmul_nbits draws them


def shifted(ctx, arr, nbytes):  # `arr` on the device, `nbytes` past the start of an allocation of its own
    base = DeviceTensor(ctx, (arr.nbytes + nbytes,), np.uint8)
    t = DeviceTensor(ctx, arr.shape, arr.dtype, ptr=base.ptr + nbytes, keepalive=base)
    t.upload(arr)
    return t


def run(ctx, lhs, quant, scales, mode=FUSED, shift=(0, 0)):
    """rten_hip_matmul_nbits_f32 under `mode` on lhs [..., rows, k] -> y [..., rows, n]; lhs and quant `shift` bytes off their allocations."""
    n, bs = quant.shape[0], 2 * quant.shape[2]
    y = DeviceTensor(ctx, list(lhs.shape[:-1]) + [n], F)
    ld, qd, sd = shifted(ctx, lhs, shift[0]), shifted(ctx, quant, shift[1]), DeviceTensor.from_numpy(ctx, scales)
    ctx.call("rten_hip_set_nbits_path", mode)
    try:
        ctx.call("rten_hip_matmul_nbits_f32", int(np.prod(lhs.shape[:-2], dtype=np.int64)), lhs.shape[-2], lhs.shape[-1], n, bs, ld.vp, qd.vp, sd.vp, y.vp)
    finally:
        ctx.call("rten_hip_set_nbits_path", AUTO)
    return y.numpy()


# one stage shorter than 64, exactly one depth block, a depth block plus a 16-deep tail, two folds with a tail, a block size larger than a stage
DEPTHS = [(16, 16), (64, 32), (256, 256), (272, 16), (528, 16), (768, 128)]


@functools.lru_cache(maxsize=None)
def case(lead, k, n, bs):
    operands = draw(lead, k, n, bs)
    return operands, ref.matmul_nbits_f32(*operands)


@pytest.fixture(params=["1", "4"])
def tile(request, monkeypatch):  # the launcher's own choice puts every shape this small on 16 x 16 tiles, so each tile is forced in turn (read at every launch)
    monkeypatch.setenv("RTEN_HIP_NBITS_TILE", request.param)
    return request.param


@pytest.mark.parametrize("k,bs", DEPTHS)
@pytest.mark.parametrize("m", [2, 15, 17, 65, (3, 5)])  # a partial 16-row tile, one row past a full tile of each kind; batch 3 x 5 rows: M is the product
def test_bits_equal_the_oracle(ctx, tile, m, k, bs):
    for n in (1, 24, 65, 130):  # partial column tiles of 16 and of 64
        operands, want = case(m if isinstance(m, tuple) else (m,), k, n, bs)
        same_bits(run(ctx, *operands), want, f"tile {tile} M {m} N {n} K {k} block {bs}")


def run_guarded(ctx, lhs, quant, scales, mode=FUSED, quant_fill=K.FILL):
    """`run` with lhs, quant, scales and y each in a tests/confine.py allocation: y one element off its 16 bytes with a full 128 x 128 tile of guard past
    the matrix, the inputs' guards NaN (quant's: `quant_fill` in every byte) -> y, confined."""
    n, bs = quant.shape[0], 2 * quant.shape[2]
    rows = int(np.prod(lhs.shape[:-1], dtype=np.int64))
    ld, qd, sd = K.Guarded(ctx, lhs), K.Guarded(ctx, quant, fill=quant_fill), K.Guarded(ctx, scales)
    guard = K.gemm_guard(n)
    yd = K.Guarded(ctx, rows * n * 4, lead=1, front=guard, back=guard)
    ctx.call("rten_hip_set_nbits_path", mode)
    try:
        ctx.call("rten_hip_matmul_nbits_f32", int(np.prod(lhs.shape[:-2], dtype=np.int64)), lhs.shape[-2], lhs.shape[-1], n, bs, ld.vp, qd.vp, sd.vp, yd.vp)
        ctx.sync()
    finally:
        ctx.call("rten_hip_set_nbits_path", AUTO)
    y = yd.check(yd.raw(), (rows, n), (n, 1), F, f"matmul_nbits rows {lhs.shape[:-1]} N {n} K {lhs.shape[-1]} block {bs}", axes=("row", "column"))
    return y.reshape(*lhs.shape[:-1], n)


@pytest.mark.parametrize("k,bs", [(16, 16), (272, 16), (768, 128)])
@pytest.mark.parametrize("m", [2, 17, 65, (3, 5)])
def test_writes_only_its_matrix(ctx, tile, m, k, bs):
    for n in (1, 24, 65, 130):
        operands, want = case(m if isinstance(m, tuple) else (m,), k, n, bs)
        for fill in K.FILLS_8BIT:  # 0xFF nibbles dequantise to a finite 7 s: a stray load of packed weights cannot hide in both fills
            same_bits(run_guarded(ctx, *operands, quant_fill=fill), want, f"tile {tile} M {m} N {n} K {k} block {bs} quant guard 0x{fill:02x}")


def test_nan_row_and_nan_scale_column_stay_put(ctx, tile):
    """A NaN row and an Inf in lhs, a NaN column and an Inf in the scales, on a shape ragged in both directions with a 16-deep tail (tile "1": the four-wave
    fold): bits against the oracle, whose result tests/test_attention_cases.py shows to differ from the finite one on exactly those rows and columns."""
    m, k, n, bs = AC.NBITS_NONFINITE_SHAPE
    (lhs, quant, scales), fin = case((m,), k, n, bs)
    bad_lhs, bad_scales, dep = AC.nbits_nonfinite(lhs, scales)
    with np.errstate(all="ignore"):
        want = ref.matmul_nbits_f32(bad_lhs, quant, bad_scales)
    got = run_guarded(ctx, bad_lhs, quant, bad_scales)
    same_bits(got, want, f"tile {tile}: non-finite rows and columns")
    same_bits(got[~dep], fin[~dep], f"tile {tile}: outside the dependency set against the finite run")


@pytest.mark.parametrize("shift", [(4, 0), (0, 1), (8, 4), (12, 7)])  # lhs off 16 bytes: dword loads; packed weights off 8 bytes: byte loads
def test_operands_off_their_vector_alignment(ctx, tile, shift):
    operands, want = case((17,), 272, 24, 16)
    same_bits(run(ctx, *operands, shift=shift), want, f"tile {tile} shift {shift}")


@pytest.mark.parametrize("m,n,k,bs", [(15, 65, 256, 256), (65, 130, 528, 16)])
def test_inside_the_forward_bound_of_an_f32_chain(ctx, m, n, k, bs):
    """|y - A W| <= (K + 2) 2^-24 (|A| |W|) per element: K FMA roundings, the dequantisation's, the block adds'.  A in [0, 1), weights symmetric."""
    rng = np.random.default_rng(7)
    lhs = rng.random((m, k), dtype=F)
    quant, scales = rng.integers(0, 256, (n, k // bs, bs // 2)).astype(np.uint8), rng.random((n, k // bs), dtype=F)
    q = np.stack([quant & 15, quant >> 4], -1).reshape(n, k // bs, bs).astype(np.float64) - 8.0
    w64 = (q * scales.astype(np.float64)[:, :, None]).reshape(n, k).T
    a64 = lhs.astype(np.float64)
    err, bound = np.abs(run(ctx, lhs, quant, scales) - a64 @ w64), (k + 2) * 2.0 ** -24 * (a64 @ np.abs(w64))
    assert (err <= bound).all(), f"{(err > bound).sum()} elements above the bound, worst ratio {np.max(err / bound):.3f}"


@pytest.mark.parametrize("band", ["sub_scales", "big_scales"])
@pytest.mark.parametrize("k,bs", [(256, 32), (144, 16)])
@pytest.mark.parametrize("rows", [2, 17])
def test_subnormal_and_overflowing_scales(ctx, rows, k, bs, band):
    c = RC.nbits_case(rows, k, bs, band)  # big_scales: 8 s overflows, (q - 8) s does not
    same_bits(run(ctx, c["lhs"], c["quant"], c["scales"]), c["want"], f"rows {rows} K {k} block {bs} {band}")


def test_modes(ctx):
    lhs, quant, scales = draw((5,), 528, 24, 16)
    want = ref.matmul_nbits_f32(lhs, quant, scales)
    for mode in (AUTO, EXPAND, FUSED):
        same_bits(run(ctx, lhs, quant, scales, mode), want, f"mode {mode}")
    one = draw((1,), 528, 24, 16, seed=5)  # rows == 1: the vector kernel and its order in every mode
    same_bits(run(ctx, *one), ref.matmul_nbits_f32(*one), "one row under mode 2")
    wide = draw((3,), 512, 4, 512)
    same_bits(run(ctx, *wide, mode=AUTO), ref.matmul_nbits_f32(*wide), "block 512 under the rule")  # kept by the older route
    for refused, code in ((lambda: run(ctx, *wide), L.ERR_UNSUPPORTED), (lambda: ctx.call("rten_hip_set_nbits_path", 7), L.ERR_INVALID_VALUE)):
        with pytest.raises(L.HipError) as e:
            refused()
        assert e.value.code == code


def test_captured_on_a_fresh_context_with_no_eager_run():
    """The MatMulNBits + Relu graph of tests/test_graph_executor.py::test_matmul_nbits_node_in_a_graph on 3 rows, recorded straight into a hipGraph on a context
    that has launched nothing: the call allocates nothing.  Three replays against the oracle."""
    rng = np.random.default_rng(17)
    quant, scales = ref.quantize_4bit_blocks((rng.standard_normal((64, 24)) * 0.1).astype(F), 16)
    x = rng.standard_normal((1, 3, 64)).astype(F)
    want = ref.relu(ref.matmul_nbits_f32(x, quant, scales))
    ctx = L.Context(0)
    try:
        xd, qd, sd = (DeviceTensor.from_numpy(ctx, a) for a in (x, quant, scales))
        h, y = DeviceTensor(ctx, want.shape, F), DeviceTensor(ctx, want.shape, F)
        ctx.call("rten_hip_set_nbits_path", FUSED)
        ctx.sync()
        ctx.graph_begin()
        ctx.call("rten_hip_matmul_nbits_f32", 1, 3, 64, 24, 16, xd.vp, qd.vp, sd.vp, h.vp)
        ctx.call("rten_hip_relu_f32", h.size, h.vp, y.vp)
        g = ctx.graph_end()
        for replay in range(3):
            y.upload(np.full(want.shape, np.nan, F))
            ctx.graph_launch(g)
            ctx.sync()
            same_bits(y.numpy(), want, f"replay {replay}")
        ctx.graph_destroy(g)
    finally:
        ctx.close()
