"""The glue operators on the device against the rules (tests/glue_rules.py) over the table of tests/glue_cases.py, every comparison of bits:

  product path, device operands   each case as a graph whose data operands are graph inputs, through rten_amd.lib.Model (the C++ executor)
  product path, host operands     the same nodes over initializers: evaluated on the host (hostops) -- the rules' bits, hence the device run's
  path flip                       the 4096 / 4097-element pairs: the same node on the two paths
  fusion modes                    one case per operator through rten_hip_run unfused, fused, and captured + replayed
  raw kernels                     the C-ABI entry points at rank 0 / 6, past the grid cap, zero sizes, signed strides, into guarded outputs

The executor behind rten_hip_model_* splits dim 0 of every input and output over its chains, so a case's graph is
    input [1, *shape] -> Squeeze(axes = [0]) -> the node under test -> Unsqueeze(axes = [0]) -> output [1, *shape]
(two views: no kernel, and a host value stays a host value); the node under test sees exactly the table's operands."""
import ctypes as C

import numpy as np
import pytest

from rten_amd import lib as L
from rten_amd import onnx_writer as ow
from rten_amd.tensor import DeviceTensor
from tests import confine as K
from tests import glue_cases as T
from tests import glue_rules as R
from tests.test_gpu_confine import guarded_in, i64, layout_check

pytestmark = pytest.mark.gpu

F, I32, I64, U8, I8 = np.float32, np.int32, np.int64, np.uint8, np.int8
ONNX_TYPE = {np.dtype(F): ow.FLOAT, np.dtype(I32): ow.INT32, np.dtype(I64): ow.INT64, np.dtype(U8): ow.UINT8, np.dtype(I8): ow.INT8}
EW_CAST, EW_NOT, EW_AND, EW_OR, EW_XOR, EW_EQUAL, EW_LESS, EW_LESS_EQ, EW_GREATER, EW_GREATER_EQ, EW_WHERE, EW_IADD, EW_ISUB, EW_IMUL, EW_IDIV = range(15)
DEV_OPS = sorted({c.op for c in T.table() if c.want_dev is not None and not c.pair and not c.id.startswith("cap-")})
HOST_OPS = sorted({c.op for c in T.table() if c.want_host is not None and not c.pair})


# ---------------------------------------------------------------------------------------------- one case as a graph
def case_graph(case, mode, prefix="", batch_views=True):
    """-> (nodes, graph inputs, initializers, feeds, output name).  `mode`: "dev" (data operands are graph inputs) or "host" (initializers)."""
    nodes, inputs, inits, feeds, names = [], [], [], {}, []
    for k, (a, place) in enumerate(zip(case.inputs, case.place)):
        name = f"{prefix}in{k}"
        if place == "input" or (place == "data" and mode == "dev"):
            if batch_views:
                inputs.append(ow.value_info(name + "_b", ONNX_TYPE[a.dtype], [1, *a.shape]))
                nodes.append(ow.node("Squeeze", [name + "_b", "axis0"], [name], name=f"{prefix}squeeze{k}"))
                feeds[name + "_b"] = a.reshape(1, *a.shape)
            else:
                inputs.append(ow.value_info(name, ONNX_TYPE[a.dtype], list(a.shape)))
                feeds[name] = a
        else:
            inits.append(ow.tensor(name, a))
        names.append(name)
    attrs = dict(case.attrs)
    if case.value is not None:
        attrs["value"] = case.value
    nodes.append(ow.node(case.op, names, [prefix + "y"], name=prefix + "node", **attrs))
    if batch_views:
        nodes.append(ow.node("Unsqueeze", [prefix + "y", "axis0"], [prefix + "y_b"], name=prefix + "unsqueeze_y"))
    return nodes, inputs, inits, feeds, prefix + ("y_b" if batch_views else "y")


def run_case(ctx, case, mode):
    """The case through rten_amd.lib.Model: -> the output array, or ("error", message)."""
    nodes, inputs, inits, feeds, out = case_graph(case, mode)
    if not inputs:  # (the executor sizes its chains from an input's dim 0)
        inputs.append(ow.value_info("unused_b", ow.FLOAT, [1, 1]))
        feeds["unused_b"] = np.zeros((1, 1), F)
    inits.append(ow.tensor("axis0", np.array([0], I64)))
    data = ow.model(nodes, inputs, [ow.value_info(out, ow.FLOAT, [])], inits)
    m = None
    try:
        m = L.Model(ctx, data)
        for name in m.inputs:
            a = feeds[name]
            p = m.bind_input(name, a.shape)
            if a.size:
                DeviceTensor(ctx, a.shape, a.dtype, ptr=p, keepalive=m).upload(a)
        m.prepare()
        m.run()
        ptr, shape = m.output(0)
        dt = np.dtype(m.output_dtype(0))
        got = DeviceTensor(ctx, shape, dt, ptr=ptr, keepalive=m).numpy() if int(np.prod(shape)) else np.zeros(shape, dt)
        assert shape[0] == 1, shape
        return got.reshape(shape[1:])
    except L.HipError as e:
        return ("error", str(e))
    finally:
        if m is not None:
            m.close()


def mismatch(case, got, want):
    """None, or what differs between a run's result and the rules' (bits; an error by its message)."""
    if isinstance(want, tuple):
        if not (isinstance(got, tuple) and want[2] in got[1]):
            return f"{case.id}: expected the refusal {want[2]!r}, got {got[1] if isinstance(got, tuple) else 'values of shape ' + str(got.shape)}"
        return None
    if isinstance(got, tuple):
        return f"{case.id}: {got[1]}"
    if not R.same_bits(got, want):
        if got.shape != want.shape or got.dtype != want.dtype:
            return f"{case.id}: {got.dtype} {got.shape} against the rules' {want.dtype} {want.shape}"
        w = np.flatnonzero(got.ravel().view(np.uint8 if got.itemsize == 1 else np.uint32) != want.ravel().view(np.uint8 if got.itemsize == 1 else np.uint32))
        return f"{case.id}: {w.size} of {got.size} elements differ, first at {w[:4].tolist()}: {got.ravel()[w[:4]]} against the rules' {want.ravel()[w[:4]]}"
    return None


def check_cases(ctx, cases, mode):
    assert cases
    wrong = [m for m in (mismatch(c, run_case(ctx, c, mode), c.want_dev if mode == "dev" else c.want_host) for c in cases) if m]
    assert not wrong, f"{len(wrong)} of {len(cases)} cases ({mode} operands):\n" + "\n".join(wrong[:40])


# ---------------------------------------------------------------------------------------------- product path
@pytest.mark.parametrize("op", DEV_OPS)
def test_product_path_with_device_operands_gives_the_rules_bits(ctx, op):
    cases = [c for c in T.table() if c.op == op and c.want_dev is not None and not c.pair and not c.id.startswith("cap-")]
    check_cases(ctx, cases, "dev")


@pytest.mark.parametrize("op", HOST_OPS)
def test_product_path_with_host_operands_gives_the_rules_bits(ctx, op):
    cases = [c for c in T.table() if c.op == op and c.want_host is not None and not c.pair]
    check_cases(ctx, cases, "host")


def test_product_path_past_the_grid_cap(ctx):
    """One case per device kernel whose grid-stride loop takes a second trip (2048 workgroups of 256 lanes, then 5 more elements)."""
    check_cases(ctx, [c for c in T.table() if c.id.startswith("cap-")], "dev")


PAIRS = sorted({c.pair for c in T.table() if c.pair})


@pytest.mark.parametrize("pair", PAIRS)
def test_path_flip_between_4096_and_4097_elements(ctx, pair):
    """An initializer of 4096 elements is a host value, one of 4097 is not: the same node on the host path and on the device path."""
    small, large = sorted((c for c in T.table() if c.pair == pair), key=lambda c: max(a.size for a in c.inputs))
    assert small.hosted and not large.hosted
    got = [run_case(ctx, c, "host") for c in (small, large)]
    wrong = [m for m in (mismatch(c, g, c.want_host) for c, g in zip((small, large), got)) if m]
    wrong += [m for m in (mismatch(c, run_case(ctx, c, "dev"), c.want_dev) for c in (small, large)) if m]
    assert not wrong, "\n".join(wrong)
    if got[0].ndim == 1 and got[1].ndim == 1 and pair not in ("concat", "slice-reverse"):  # element-wise: the shared prefix, bit for bit
        assert R.same_bits(got[0], got[1][:T.HOST_CONST]), pair


# ---------------------------------------------------------------------------------------------- fusion modes
def test_fusion_modes_agree_on_one_case_per_operator(ctx, tmp_path):
    """One graph holding one case per operator, through rten_hip_run unfused, fused, and captured into a hipGraph and replayed three times: the
    host-evaluated steps stay out of the capture, the device steps replay, and all three give the rules' bits."""
    from tests.test_graph_executor import run_cli
    from tests.test_gpu_math_pad import GRAPH_MODES
    nodes, inputs, inits, feeds, outs = [], [], [], {}, {}
    for k, cid in enumerate(T.FUSION_SUBSET):
        c = T.by_id(cid)
        mode = "dev" if c.want_dev is not None else "host"
        n, i, t, f, out = case_graph(c, mode, prefix=f"c{k}_", batch_views=False)
        nodes += n; inputs += i; inits += t; feeds.update(f)
        outs[out] = c.want_dev if mode == "dev" else c.want_host
    data = ow.model(nodes, inputs, [ow.value_info(o, ow.FLOAT, []) for o in outs], inits)
    (tmp_path / "m.onnx").write_bytes(data)
    args = []
    for name, a in feeds.items():
        np.ascontiguousarray(a).tofile(tmp_path / f"{name}.bin")
        args += ["--input", f"{name}={tmp_path / (name + '.bin')}"]
    for flags in GRAPH_MODES:
        dumps = []
        for o in outs:
            dumps += ["--dump", f"{o}={tmp_path / (o + '.bin')}"]
        r = run_cli(*flags, *args, *dumps, str(tmp_path / "m.onnx"))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        if "--graph" in flags:
            assert "Captured the plan into a hipGraph" in r.stdout
        wrong = []
        for (o, want), cid in zip(outs.items(), T.FUSION_SUBSET):
            got = np.fromfile(tmp_path / (o + ".bin"), want.dtype)
            if got.size != want.size or not R.same_bits(got.reshape(want.shape), want):
                wrong.append(f"{cid} ({' '.join(flags) or 'fused'})")
        assert not wrong, wrong


# ---------------------------------------------------------------------------------------------- raw kernels
def strict(ctx, what, ins, want, call):
    """layout_check (guarded outputs at leads 0, 1, 3: every byte outside the output keeps its fill), then the bits themselves -- the sign of a zero
    and a NaN's payload included, which layout_check's comparison lets pass."""
    layout_check(ctx, what, ins, want, call)
    gs = [guarded_in(ctx, a) for a in ins]
    y = DeviceTensor(ctx, want.shape, want.dtype)
    call(*[g.vp for g in gs], C.c_void_p(y.ptr))
    ctx.sync()
    assert R.same_bits(y.numpy(), want), what


def writes_nothing(ctx, what, call):
    """A zero-size launch returns OK and leaves a guarded buffer at its fill."""
    out = K.Guarded(ctx, 64)
    call(out.vp)
    ctx.sync()
    assert (out.raw() == K.FILL).all(), what


def refused(ctx, match, name, *args):
    with pytest.raises(L.HipError, match=match):
        ctx.call(name, *args)


def nd_call(ctx, op, shape, dts, strides, y_dt):
    """rten_hip_elementwise_nd over up to three operands given as (dtype codes, strides)."""
    def call(*ptrs):
        *ins, y = ptrs
        a, b, c = (list(ins) + [None, None])[:3]
        sa, sb, sc = (list(strides) + [None, None])[:3]
        ctx.call("rten_hip_elementwise_nd", op, len(shape), i64(shape), a, dts[0], i64(sa), b, dts[1] if len(dts) > 1 else 0, i64(sb) if sb is not None else None, c,
                 i64(sc) if sc is not None else None, y, y_dt)
    return call


def bstrides(shape, out):
    """Element strides of a `shape` operand broadcast over `out` (0 on broadcast axes)."""
    st, acc = [0] * len(out), 1
    for i in range(len(shape) - 1, -1, -1):
        st[len(out) - len(shape) + i] = 0 if shape[i] == 1 else acc
        acc *= shape[i]
    return st


RANK6 = ((2, 3, 1, 2, 1, 2), (1, 3, 2, 1, 3, 2), (2, 3, 2, 2, 3, 2))
SEVEN = (1,) * 7


def test_raw_elementwise_nd(ctx):
    rng = np.random.default_rng(5)
    # rank 0, rank 6 with both operands broadcast, one trip past the grid cap
    for sa, sb, so in (((), (), ()), RANK6, ((T.PAST_CAP,), (1,), (T.PAST_CAP,))):
        a, b = rng.integers(-2**31, 2**31, sa).astype(I32), rng.integers(-2**31, 2**31, sb).astype(I32)
        strict(ctx, f"iadd {sa} {sb}", [a, b], R.iarith("Add", a, b).reshape(so), nd_call(ctx, EW_IADD, so, (L.DT_I32, L.DT_I32), (bstrides(sa, so), bstrides(sb, so)), L.DT_I32))
    a, b = np.array([T.I32_MIN, -7, 7, 0, 9], I32), np.array([-1, 2, -2, 5, 0], I32)
    strict(ctx, "idiv", [a, b], R.idiv_device(a, b), nd_call(ctx, EW_IDIV, (5,), (L.DT_I32, L.DT_I32), ((1,), (1,)), L.DT_I32))
    # Where moves 4-byte words: payloads and the sign of zero survive
    c = rng.integers(0, 2, (2, 1, 4)).astype(I32)
    x = np.array([0x7FA00001, 0xFFC12345, 0x80000000], np.uint32).view(F).reshape(1, 3, 1)
    y = np.array([0x00000001, 0x7F800000, 0x80000000, 0x7FC00000], np.uint32).view(F)
    strict(ctx, "where", [c, x, y], R.where(c, x, y), nd_call(ctx, EW_WHERE, (2, 3, 4), (L.DT_I32, L.DT_F32), ((4, 0, 1), (0, 1, 0), (0, 0, 1)), L.DT_F32))
    # signed strides: shape (5, 7), strides (-7, -1), base at the last element -- the form slice_tensor launches for a negative step (x + 0 moves the word)
    m = np.concatenate([np.array([-0.0, T.NAN_PAYLOAD], F), rng.standard_normal(33).astype(F)]).reshape(5, 7)
    zero = np.zeros((), I32)
    for lead in (0, 1, 3):
        g, z, out = guarded_in(ctx, m, lead), guarded_in(ctx, zero), K.Guarded(ctx, m.nbytes, lead=lead)
        ctx.call("rten_hip_elementwise_nd", EW_IADD, 2, i64((5, 7)), C.c_void_p(g.ptr + 4 * 34), L.DT_I32, i64((-7, -1)), z.vp, L.DT_I32, i64((0, 0)), None, None, out.vp, L.DT_I32)
        ctx.sync()
        assert R.same_bits(out.check(out.raw(), (5, 7), (7, 1), F, "signed strides"), m[::-1, ::-1])
    # 8-bit operands read through strides from odd byte addresses: every code, every second byte of a buffer that starts one byte off alignment
    codes = np.arange(256, dtype=U8)
    wide = np.stack([codes, codes[::-1]], 1).reshape(-1)  # the codes at the even bytes
    for src, src_dt in ((wide, L.DT_U8), (wide.view(I8), L.DT_I8)):
        for to, to_dt in ((F, L.DT_F32), (I32, L.DT_I32), (U8, L.DT_U8), (I8, L.DT_I8)):
            if to == src.dtype.type:
                continue
            want = R.cast(src[::2], to)
            for lead in (1, 3):
                g, out = guarded_in(ctx, src, lead), K.Guarded(ctx, want.nbytes, lead=lead, itemsize=want.itemsize)
                assert g.ptr % 2 == 1
                ctx.call("rten_hip_elementwise_nd", EW_CAST, 2, i64((16, 16)), g.vp, src_dt, i64((32, 2)), None, 0, None, None, None, out.vp, to_dt)
                ctx.sync()
                assert R.same_bits(out.check(out.raw(), (256,), (1,), to, f"cast {src.dtype} -> {np.dtype(to)}"), want)
    f = np.array([2147483520.0, 2147483648.0, -2147483648.0, 3e10, -3e10, np.nan, 0.9, -0.9, 255.5, 256.0, 127.9, -128.9, -129.0], F)
    for to, to_dt in ((I32, L.DT_I32), (U8, L.DT_U8), (I8, L.DT_I8)):
        strict(ctx, f"cast f32 -> {np.dtype(to)}", [f], R.cast(f, to), nd_call(ctx, EW_CAST, f.shape, (L.DT_F32,), ((1,),), to_dt))
    # zero size: OK, nothing written; rank 7: refused with a message, no launch
    a = guarded_in(ctx, np.zeros(4, I32))
    writes_nothing(ctx, "iadd (3, 0, 4)", lambda yv: ctx.call("rten_hip_elementwise_nd", EW_IADD, 3, i64((3, 0, 4)), a.vp, L.DT_I32, i64((0, 4, 1)), a.vp, L.DT_I32, i64((0, 0, 1)), None, None, yv, L.DT_I32))
    refused(ctx, "more than 6 dims", "rten_hip_elementwise_nd", EW_IADD, 7, i64(SEVEN), a.vp, L.DT_I32, i64(SEVEN), a.vp, L.DT_I32, i64(SEVEN), None, None, a.vp, L.DT_I32)


def test_raw_transpose_and_copy_strided(ctx):
    rng = np.random.default_rng(6)
    for shape, perm in (((), ()), ((2, 3, 1, 2, 3, 2), (5, 3, 4, 0, 2, 1)), ((T.PAST_CAP // 3 + 1, 3), (1, 0))):
        x = rng.standard_normal(shape).astype(F)
        strict(ctx, f"transpose {shape}", [x], R.transpose(x, perm or None), lambda xv, yv: ctx.call("rten_hip_transpose_b32", len(shape), i64(shape), (C.c_int32 * max(len(perm), 1))(*perm), xv, yv))
    for shape, strides, src in (((), (), (1,)), ((2, 3, 2, 2, 3, 2), (6, 0, 0, 3, 1, 0), (12,)), ((T.PAST_CAP,), (0,), (1,)), ((3, T.PAST_CAP // 3 + 1), (1, 3), (T.PAST_CAP + 3,))):
        x = rng.standard_normal(src).astype(F)
        want = np.array(np.lib.stride_tricks.as_strided(x, shape, [4 * s for s in strides]), order="C")
        strict(ctx, f"copy_strided {shape} {strides}", [x], want, lambda xv, yv: ctx.call("rten_hip_copy_strided_b32", len(shape), i64(shape), i64(strides), xv, yv))
    x = guarded_in(ctx, np.zeros(12, F))
    writes_nothing(ctx, "transpose (3, 0, 4)", lambda yv: ctx.call("rten_hip_transpose_b32", 3, i64((3, 0, 4)), (C.c_int32 * 3)(2, 0, 1), x.vp, yv))
    writes_nothing(ctx, "copy_strided (3, 0, 4)", lambda yv: ctx.call("rten_hip_copy_strided_b32", 3, i64((3, 0, 4)), i64((4, 0, 1)), x.vp, yv))
    refused(ctx, "at most 6 dims", "rten_hip_transpose_b32", 7, i64(SEVEN), (C.c_int32 * 7)(*range(7)), x.vp, x.vp)
    refused(ctx, "at most 6 dims", "rten_hip_copy_strided_b32", 7, i64(SEVEN), i64(SEVEN), x.vp, x.vp)
    # negative strides stay refused here (slice_tensor sends them to rten_hip_elementwise_nd)
    refused(ctx, "copy_strided: bad dimension", "rten_hip_copy_strided_b32", 2, i64((3, 4)), i64((-4, -1)), C.c_void_p(x.ptr + 44), x.vp)


def test_raw_binary_broadcast(ctx):
    rng = np.random.default_rng(7)
    for sa, sb, so in (((), (), ()), RANK6, ((T.PAST_CAP,), (1,), (T.PAST_CAP,)), ((3, 1), (1, 5), (3, 5))):
        a, b = rng.standard_normal(sa).astype(F), (rng.standard_normal(sb).astype(F) + F(3))
        for op, want in ((L.BINARY_ADD, R.farith("Add", a, b)), (L.BINARY_MUL, R.farith("Mul", a, b)), (L.BINARY_SUB, R.farith("Sub", a, b)),
                         (L.BINARY_DIV, np.divide(*np.broadcast_arrays(a, b)).astype(F))):  # the raw ABI's op 3 is a TRUE division, also by one element
            strict(ctx, f"binary_broadcast op {op} {sa} {sb}", [a, b], want.reshape(so),
                   lambda av, bv, yv: ctx.call("rten_hip_binary_broadcast_f32", op, len(so), i64(so), i64(bstrides(sa, so)), i64(bstrides(sb, so)), av, bv, yv))
    a, b = rng.standard_normal(4096).astype(F), np.array([3.0], F)
    strict(ctx, "div_f32 by one element", [a, b], (a / b).astype(F), lambda av, bv, yv: ctx.call("rten_hip_div_f32", a.size, av, bv, 1, yv))
    x = guarded_in(ctx, np.ones(4, F))
    writes_nothing(ctx, "binary_broadcast (3, 0, 4)", lambda yv: ctx.call("rten_hip_binary_broadcast_f32", 0, 3, i64((3, 0, 4)), i64((0, 0, 1)), i64((0, 0, 1)), x.vp, x.vp, yv))
    refused(ctx, "at most 6 dims", "rten_hip_binary_broadcast_f32", 0, 7, i64(SEVEN), i64(SEVEN), i64(SEVEN), x.vp, x.vp, x.vp)


def test_raw_gather_and_copy_rows(ctx):
    rng = np.random.default_rng(8)
    x = rng.standard_normal((2, 3, 1, 2, 3, 2)).astype(F)
    ids = np.array([2, -1, 0, 7, -9], I32)  # two out of range: clamped (include/rten_hip.h)
    strict(ctx, "gather_axis rank 6, axis 4", [x, ids], R.gather_device(x, ids, 4), lambda xv, iv, yv: ctx.call("rten_hip_gather_axis_b32", 12, 3, 2, ids.size, xv, iv, yv))
    tab_i, tab_f = rng.integers(-9, 9, (6,)).astype(I32), rng.standard_normal((6, 1)).astype(F)
    big = rng.integers(-8, 8, (T.PAST_CAP,)).astype(I32)
    strict(ctx, "gather_axis past the cap", [tab_i, big], R.gather_device(tab_i, big, 0), lambda xv, iv, yv: ctx.call("rten_hip_gather_axis_b32", 1, 6, 1, big.size, xv, iv, yv))
    strict(ctx, "gather_rows past the cap", [tab_f, big], R.gather_device(tab_f, big, 0), lambda xv, iv, yv: ctx.call("rten_hip_gather_rows_f32", big.size, 1, 6, xv, iv, yv))
    one = np.array(4, I32)
    strict(ctx, "gather_axis, one scalar id", [tab_i, one], R.gather(tab_i, one, 0), lambda xv, iv, yv: ctx.call("rten_hip_gather_axis_b32", 1, 6, 1, 1, xv, iv, yv))
    rows = rng.standard_normal((3, T.PAST_CAP // 3 + 1)).astype(F)
    strict(ctx, "copy_rows past the cap", [rows], rows, lambda sv, yv: ctx.call("rten_hip_copy_rows_b32", rows.shape[0], rows.shape[1], sv, rows.shape[1], yv, rows.shape[1]))
    strict(ctx, "copy_rows, one element", [rows[:1, :1]], rows[:1, :1].copy(), lambda sv, yv: ctx.call("rten_hip_copy_rows_b32", 1, 1, sv, 1, yv, 1))
    t, i = guarded_in(ctx, tab_f), guarded_in(ctx, ids)
    writes_nothing(ctx, "gather_axis, no ids", lambda yv: ctx.call("rten_hip_gather_axis_b32", 3, 2, 1, 0, t.vp, i.vp, yv))
    writes_nothing(ctx, "gather_axis, inner 0", lambda yv: ctx.call("rten_hip_gather_axis_b32", 3, 2, 0, 5, t.vp, i.vp, yv))
    writes_nothing(ctx, "gather_rows, no ids", lambda yv: ctx.call("rten_hip_gather_rows_f32", 0, 1, 6, t.vp, i.vp, yv))
    writes_nothing(ctx, "copy_rows, no rows", lambda yv: ctx.call("rten_hip_copy_rows_b32", 0, 4, t.vp, 4, yv, 4))
    writes_nothing(ctx, "copy_rows, empty rows", lambda yv: ctx.call("rten_hip_copy_rows_b32", 3, 0, t.vp, 0, yv, 0))
