"""QuantizeLinear, DequantizeLinear and their fused round trip on the device against tests/qdq_rules.py, bit for bit: the C ABI (sizes, views at every
misalignment, the grid-stride loop, per-axis geometries, out-of-domain inputs), the Python and C++ host operators on the reference's literal cases, and
two statically quantised graphs (QDQ layout) through the resident executor -- unfused, fused, captured into a hipGraph and on a replica -- against the
composition of the rules with the CPU oracle's operators."""
import collections
import ctypes as C
import re

import numpy as np
import pytest

from oracle import ref
from rten_amd import lib as L
from rten_amd import ops
from rten_amd.tensor import DeviceTensor
from tests import qdq_rules as Q
from tests.test_qdq_ops import GOLDEN, encoder_qdq, golden_operands

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4099]
DT = {np.dtype(np.uint8): L.DT_U8, np.dtype(np.int8): L.DT_I8, np.dtype(np.int32): L.DT_I32}
ZP = {np.dtype(np.uint8): 131, np.dtype(np.int8): -7, np.dtype(np.int32): 1000}
GUARD = 0xAB


def bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = got.view(np.uint8) == want.view(np.uint8) if got.dtype.itemsize == 1 else got.view(np.int32) == want.view(np.int32)
    if not same.all():
        at = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {(~same).sum()} of {same.size} values differ, first at {at}: {got[at]!r} vs {want[at]!r}")


def f32_inputs(n, scale, seed=0):
    """Inside the contract domain: products around +-200 (both saturation ends of either type are reached), exact ties, -0.0, and a few products near 1e6."""
    rng = np.random.default_rng(1000 + n + seed)
    x = (rng.standard_normal(n) * 200 * F(scale)).astype(F)
    pins = (np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -0.0, 0.0, 1e6, -1e6, 254.5, 255.5, -128.5, 127.5], F) * F(scale)).astype(F)
    k = min(n, pins.size)
    x[:k] = pins[:k]
    if n > 2 * pins.size:
        x[-pins.size:] = pins[::-1]  # the tail elements too
    return x


def quantized_inputs(n, dtype, seed=0):
    rng = np.random.default_rng(2000 + n + seed)
    dtype = np.dtype(dtype)
    if dtype == np.int32:
        x = rng.integers(-(2 ** 31), 2 ** 31, n).astype(np.int32)
        pins = np.array([2 ** 24 + 1, -(2 ** 24) - 3, 2 ** 31 - 1, -(2 ** 31), 0, 2 ** 25 + 2], np.int32)  # rounded conversions and the wrapping subtraction
        x[:min(n, pins.size)] = pins[:min(n, pins.size)]
        return x
    info = np.iinfo(dtype)
    x = rng.integers(info.min, info.max + 1, n).astype(dtype)
    x[:min(n, 2)] = np.array([info.min, info.max], dtype)[:min(n, 2)]
    return x


def view_of(ctx, arr, byte_offset, guard_bytes=16):
    """`arr` uploaded `byte_offset` bytes past an allocation, with GUARD bytes before and behind: -> (view, whole buffer)."""
    raw = np.full(byte_offset + arr.nbytes + guard_bytes, GUARD, np.uint8)
    raw[byte_offset:byte_offset + arr.nbytes] = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = DeviceTensor.from_numpy(ctx, raw)
    return DeviceTensor(ctx, arr.shape, arr.dtype, ptr=buf.ptr + byte_offset, keepalive=buf), buf


def read_view(view, buf, byte_offset):
    raw = buf.numpy()
    n = view.size * np.dtype(view.dtype).itemsize
    assert (raw[:byte_offset] == GUARD).all() and (raw[byte_offset + n:] == GUARD).all(), "wrote outside y"
    return raw[byte_offset:byte_offset + n].view(view.dtype).reshape(view.shape).copy()


def params(ctx, scale, zp):
    sd = DeviceTensor.from_numpy(ctx, np.asarray(scale, F))
    zd = None if zp is None else DeviceTensor.from_numpy(ctx, np.asarray(zp))
    return sd, zd


def call(ctx, fn, dtype, geometry, x, scale, zp, out_dtype, x_off=0, y_off=0, in_place=False):
    """One launch of an entry point on views `x_off` / `y_off` BYTES past their allocations; `geometry` = (outer, channels, inner)."""
    sd, zd = params(ctx, scale, zp)
    xv, xbuf = view_of(ctx, x, x_off)
    if in_place:
        yv, ybuf, y_off = xv, xbuf, x_off
    else:
        yv, ybuf = view_of(ctx, np.zeros(x.shape, out_dtype), y_off)
    ctx.call(fn, DT[np.dtype(dtype)], *geometry, xv.vp, sd.vp, None if zd is None else zd.vp, yv.vp)
    ctx.sync()
    return read_view(yv, ybuf, y_off)


def quantize(ctx, x, scale, zp, dtype, geometry=None, **kw):
    return call(ctx, "rten_hip_quantize_linear_f32", dtype, geometry or (1, 1, x.size), x, scale, zp, dtype, **kw)


def dequantize(ctx, x, scale, zp, geometry=None, **kw):
    return call(ctx, "rten_hip_dequantize_linear_f32", x.dtype, geometry or (1, 1, x.size), x, scale, zp, np.float32, **kw)


def round_trip(ctx, x, scale, zp, dtype, geometry=None, **kw):
    return call(ctx, "rten_hip_quantize_dequantize_f32", dtype, geometry or (1, 1, x.size), x, scale, zp, np.float32, **kw)


# ---------------------------------------------------------------------------------------------- the C ABI, per-tensor
@pytest.mark.parametrize("with_zp", [True, False], ids=["zp", "no-zp"])
@pytest.mark.parametrize("dtype", [np.uint8, np.int8], ids=["u8", "i8"])
def test_quantize_sizes(ctx, dtype, with_zp):
    """n: 1 / 3 scalar only, 4 one vector, 5 vector + tail, 15..17 / 63..65 / 255..257 around a wave's and a workgroup's vectors, 4099 several workgroups + tail."""
    scale = np.array(0.05, F)
    zp = np.array(ZP[np.dtype(dtype)], dtype) if with_zp else None
    for n in SIZES:
        x = f32_inputs(n, scale)
        want = Q.quantize_linear(x, scale, zp, dtype=dtype)
        bits_equal(quantize(ctx, x, scale, zp, dtype), want, f"quantize n {n}")
        # the fused round trip gives the bits of the two kernels run in sequence, out of place and with y == x
        two = dequantize(ctx, quantize(ctx, x, scale, zp, dtype), scale, zp)
        bits_equal(two, Q.quantize_dequantize(x, scale, zp, dtype=dtype), f"quantize then dequantize n {n}")
        bits_equal(round_trip(ctx, x, scale, zp, dtype), two, f"round trip n {n}")
        bits_equal(round_trip(ctx, x, scale, zp, dtype, in_place=True), two, f"round trip in place n {n}")


@pytest.mark.parametrize("with_zp", [True, False], ids=["zp", "no-zp"])
@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.int32], ids=["u8", "i8", "i32"])
def test_dequantize_sizes(ctx, dtype, with_zp):
    scale = np.array(0.0371, F)
    zp = np.array(ZP[np.dtype(dtype)], dtype) if with_zp else None
    for n in SIZES:
        x = quantized_inputs(n, dtype)
        bits_equal(dequantize(ctx, x, scale, zp), Q.dequantize_linear(x, scale, zp), f"dequantize n {n}")
    if np.dtype(dtype) == np.int32:  # the subtraction wraps
        x = np.array([2 ** 31 - 1, -(2 ** 31), 5], np.int32)
        z = np.array(-1, np.int32)
        got = dequantize(ctx, x, np.array(1.0, F), z)
        bits_equal(got, Q.dequantize_linear(x, np.array(1.0, F), z), "wrapping subtraction")
        assert got.tolist() == [-(2.0 ** 31), -(2.0 ** 31), 6.0]


@pytest.mark.parametrize("f32_off", [0, 1, 2, 3])
@pytest.mark.parametrize("u8_off", [0, 1, 2, 3])
def test_views_at_every_misalignment(ctx, f32_off, u8_off):
    """The f32 operand `f32_off` elements and the 8-bit operand `u8_off` bytes past a 16-byte boundary: a scalar head, vectors and a scalar tail where one
    head aligns both, the per-element form otherwise; nothing is written outside y (guard bytes on both sides)."""
    n = 1030
    scale, zp = np.array(0.05, F), np.array(131, np.uint8)
    x = f32_inputs(n, scale, seed=f32_off)
    bits_equal(quantize(ctx, x, scale, zp, np.uint8, x_off=4 * f32_off, y_off=u8_off), Q.quantize_linear(x, scale, zp), "quantize on views")
    xq = quantized_inputs(n, np.int8, seed=u8_off)
    zi = np.array(-7, np.int8)
    bits_equal(dequantize(ctx, xq, scale, zi, x_off=u8_off, y_off=4 * f32_off), Q.dequantize_linear(xq, scale, zi), "dequantize on views")
    # round trip: x at f32_off elements, y at u8_off ELEMENTS (both f32), and in place
    want = Q.quantize_dequantize(x, scale, zp)
    bits_equal(round_trip(ctx, x, scale, zp, np.uint8, x_off=4 * f32_off, y_off=4 * u8_off), want, "round trip on views")
    bits_equal(round_trip(ctx, x, scale, zp, np.uint8, x_off=4 * f32_off, in_place=True), want, "round trip in place on a view")
    x32 = quantized_inputs(n, np.int32, seed=f32_off)
    z32 = np.array(1000, np.int32)
    bits_equal(dequantize(ctx, x32, scale, z32, x_off=4 * f32_off, y_off=4 * u8_off), Q.dequantize_linear(x32, scale, z32), "int32 dequantize on views")


def test_grid_stride_above_the_grid_cap(ctx):
    n = 2 ** 21 + 5  # 4 elements per lane, 256 lanes, 2048 workgroups = 2^21: the loop's second trip and an odd tail
    scale, zp = np.array(0.05, F), np.array(100, np.uint8)
    x = f32_inputs(n, scale)
    q = Q.quantize_linear(x, scale, zp)
    bits_equal(quantize(ctx, x, scale, zp, np.uint8), q, "quantize")
    bits_equal(round_trip(ctx, x, scale, zp, np.uint8), Q.dequantize_linear(q, scale, zp), "round trip")
    bits_equal(dequantize(ctx, q, scale, zp), Q.dequantize_linear(q, scale, zp), "dequantize")


# ---------------------------------------------------------------------------------------------- the C ABI, per-axis
PER_AXIS = [((2, 3, 5), 0), ((2, 3, 5), 1), ((2, 3, 5), 2), ((2, 3, 5), -1), ((1, 4, 1), 1), ((6, 7), 1), ((2, 3, 1030), 1),
            ((5, 8), 1), ((40, 260), 1), ((3, 4, 16), 1)]  # (also: inner == 1 with channels % 4 == 0 -- the 4-channel lanes -- and aligned planes)


@pytest.mark.parametrize("shape, axis", PER_AXIS, ids=[f"{'x'.join(map(str, s))}-axis{a}" for s, a in PER_AXIS])
def test_per_axis(ctx, shape, axis):
    ax = axis % len(shape)
    ch = shape[ax]
    geometry = (int(np.prod(shape[:ax], dtype=np.int64)), ch, int(np.prod(shape[ax + 1:], dtype=np.int64)))
    rng = np.random.default_rng(ch * 31 + len(shape))
    scale = rng.uniform(0.01, 0.2, ch).astype(F)
    bshape = [1] * len(shape)
    bshape[ax] = ch
    x = (f32_inputs(int(np.prod(shape)), 1.0).reshape(shape) * scale.reshape(bshape)).astype(F)
    for dtype in (np.uint8, np.int8):
        info = np.iinfo(dtype)
        zp = rng.integers(info.min, info.max + 1, ch).astype(dtype)
        zp[0] = info.max
        for z in (zp, None):
            q = Q.quantize_linear(x, scale, z, axis=axis, dtype=dtype)
            bits_equal(quantize(ctx, x, scale, z, dtype, geometry), q, f"quantize {np.dtype(dtype).name}")
            d = Q.dequantize_linear(q, scale, z, axis=axis)
            bits_equal(dequantize(ctx, q, scale, z, geometry), d, f"dequantize {np.dtype(dtype).name}")
            bits_equal(round_trip(ctx, x, scale, z, dtype, geometry), d, f"round trip {np.dtype(dtype).name}")
            bits_equal(round_trip(ctx, x, scale, z, dtype, geometry, in_place=True), d, f"round trip in place {np.dtype(dtype).name}")
    x32 = quantized_inputs(x.size, np.int32).reshape(shape)
    z32 = rng.integers(-1000, 1000, ch).astype(np.int32)
    bits_equal(dequantize(ctx, x32, scale, z32, geometry), Q.dequantize_linear(x32, scale, z32, axis=axis), "dequantize int32")
    # a view one byte / one element off: planes and rows lose their common alignment
    zp = np.full(ch, 3, np.uint8)
    bits_equal(quantize(ctx, x, scale, zp, np.uint8, geometry, x_off=4, y_off=1), Q.quantize_linear(x, scale, zp, axis=axis), "quantize on a view")


def test_out_of_domain_inputs_follow_the_documented_rule(ctx):
    """NaN, +-inf and products beyond 2^31: u8 per-tensor follows the vector kernel's statement (dql::quant_u8: all 0), every other form the scalar
    definition (a saturating cast, NaN -> 0).  docs/KERNELS.md 4.9."""
    scale = np.array(0.05, F)
    x = np.tile(np.array([np.nan, np.inf, -np.inf, 3e9 * 0.05, -3e9 * 0.05, 1.0], F), 11)  # vectors and a tail
    zp8, zi8 = np.array(7, np.uint8), np.array(-7, np.int8)
    got = quantize(ctx, x, scale, zp8, np.uint8)
    bits_equal(got, Q.quantize_linear(x, scale, zp8), "u8 per-tensor")
    assert got[:6].tolist() == [0, 0, 0, 0, 0, 27]
    got = quantize(ctx, x, scale, zi8, np.int8)
    bits_equal(got, Q.quantize_linear(x, scale, zi8), "i8 per-tensor")
    assert got[:6].tolist() == [0, 127, -128, 127, -128, 13]
    xa = x.reshape(11, 6)
    sa, za = np.full(6, 0.05, F), np.full(6, 7, np.uint8)
    got = quantize(ctx, xa, sa, za, np.uint8, (11, 6, 1))
    bits_equal(got, Q.quantize_linear(xa, sa, za, axis=1), "u8 per-axis")
    assert got[0].tolist() == [0, 255, 0, 255, 0, 27]
    bits_equal(round_trip(ctx, x, scale, zp8, np.uint8), Q.quantize_dequantize(x, scale, zp8), "round trip u8")
    bits_equal(round_trip(ctx, x, scale, zi8, np.int8), Q.quantize_dequantize(x, scale, zi8), "round trip i8")
    # a zero scale: 1 / 0 = inf, the products are +-inf or NaN
    zero = np.array(0.0, F)
    xs = np.array([1.0, -1.0, 0.0, 5.0, -0.0], F)
    bits_equal(quantize(ctx, xs, zero, zi8, np.int8), Q.quantize_linear(xs, zero, zi8), "zero scale")


def test_bad_arguments_are_errors(ctx):
    x = DeviceTensor.from_numpy(ctx, np.zeros(8, F))
    s = DeviceTensor.from_numpy(ctx, np.ones(1, F))
    y = DeviceTensor.from_numpy(ctx, np.zeros(8, np.uint8))
    lib = ctx.lib
    i64 = C.c_int64
    assert lib.rten_hip_quantize_linear_f32(ctx.h, L.DT_I32, i64(1), i64(1), i64(8), x.vp, s.vp, None, y.vp) != L.OK  # int32 is a dequantize-only type
    assert lib.rten_hip_dequantize_linear_f32(ctx.h, L.DT_F32, i64(1), i64(1), i64(8), y.vp, s.vp, None, x.vp) != L.OK
    assert lib.rten_hip_quantize_linear_f32(ctx.h, L.DT_U8, i64(1), i64(0), i64(8), x.vp, s.vp, None, y.vp) != L.OK
    assert lib.rten_hip_quantize_linear_f32(ctx.h, L.DT_U8, i64(1), i64(1), i64(8), C.c_void_p(x.ptr + 2), s.vp, None, y.vp) != L.OK  # an f32 operand off its alignment
    assert lib.rten_hip_quantize_linear_f32(ctx.h, L.DT_U8, i64(0), i64(3), i64(8), None, None, None, None) == L.OK  # empty: nothing to do


# ---------------------------------------------------------------------------------------------- both host layers on the reference's literal cases
@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_python_operators_on_the_reference_cases(ctx, case):
    x, scale, zp = golden_operands(case)
    dev = lambda a: None if a is None else DeviceTensor.from_numpy(ctx, a)
    inputs = [dev(x), dev(scale), dev(zp)]
    if "error" in case:
        with pytest.raises(ops.OpError) as e:
            ops.DequantizeLinear(axis=case["axis"]).run(ctx, inputs)
        assert (e.value.kind, e.value.msg) == (case["error"]["kind"], case["error"]["msg"])
        return
    want = np.array(case["expected"], F).reshape(x.shape)
    y = ops.DequantizeLinear(axis=case["axis"]).run(ctx, inputs)[0]
    bits_equal(y.numpy(), want, "DequantizeLinear")
    back = ops.QuantizeLinear(axis=case["axis"], output_dtype=x.dtype).run(ctx, [y, inputs[1], inputs[2]])[0]
    bits_equal(back.numpy(), x, "QuantizeLinear of the result")


def _one_node_graph(case, x, scale, zp):
    """DequantizeLinear of a graph INPUT (a constant would be folded at load) followed by QuantizeLinear of the result: the C++ host operators."""
    from rten_amd import onnx_writer as ow
    code = ow._NP2ONNX[x.dtype]
    inits = [ow.tensor("s", scale)] + ([] if zp is None else [ow.tensor("z", zp)])
    tail = [] if zp is None else ["z"]
    nodes = [ow.node("DequantizeLinear", ["x", "s"] + tail, ["y"], name="dq_node", axis=case["axis"]),
             ow.node("QuantizeLinear", ["y", "s"] + tail, ["back"], name="q_node", axis=case["axis"], **({} if zp is not None else {"output_dtype": code}))]
    return ow.model(nodes, [ow.value_info("x", code, list(x.shape))], [ow.value_info("y", ow.FLOAT, list(x.shape)), ow.value_info("back", code, list(x.shape))], inits, opset=21)


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_cpp_operators_on_the_reference_cases(tmp_path, case):
    from tests.test_graph_executor import run_cli
    x, scale, zp = golden_operands(case)
    model, xin, yout, bout = tmp_path / "m.onnx", tmp_path / "x.bin", tmp_path / "y.bin", tmp_path / "back.bin"
    model.write_bytes(_one_node_graph(case, x, scale, zp))
    xin.write_bytes(x.tobytes())
    out = run_cli("--input", f"x={xin}", "--dump", f"y={yout}", "--dump", f"back={bout}", str(model))
    if "error" in case:
        assert out.returncode != 0 and case["error"]["msg"] in out.stderr and "dq_node" in out.stderr, out.stderr + out.stdout
        return
    assert out.returncode == 0, out.stderr + out.stdout
    bits_equal(np.fromfile(yout, F).reshape(x.shape), np.array(case["expected"], F).reshape(x.shape), "DequantizeLinear")
    bits_equal(np.fromfile(bout, x.dtype).reshape(x.shape), x, "QuantizeLinear of the result")


# ---------------------------------------------------------------------------------------------- statically quantised graphs through the resident executor
def cli_run(tmp_path, data, inputs, out_name, out_dtype, *flags, sizes=None):
    from tests.test_graph_executor import run_cli
    model, yout = tmp_path / "m.onnx", tmp_path / "y.bin"
    model.write_bytes(data)
    args = []
    for name, a in inputs.items():
        f = tmp_path / f"{name}.bin"
        f.write_bytes(np.ascontiguousarray(a).tobytes())
        args += ["--input", f"{name}={f}"]
    for k, v in (sizes or {}).items():
        args += ["-s", f"{k}={v}"]
    out = run_cli(*flags, *args, "--dump", f"{out_name}={yout}", str(model))
    assert out.returncode == 0, out.stderr + out.stdout
    return np.fromfile(yout, out_dtype), out.stdout


def step_kinds(report):
    """{step kind: count} from the per-operator table of rten_hip_run -t."""
    kinds = collections.Counter()
    for line in report.split("Operator timing")[1].splitlines()[1:]:
        m = re.match(r"^\s{4}(\S.*?)\s+x(\d+)\s+[\d.]+ms", line)
        if m:
            kinds[m.group(1)] += int(m.group(2))
    return kinds


def model_outputs(ctx, data, feeds, out_dtype):
    """The plan executor behind the C ABI (captured into a hipGraph by prepare) and a replica of it on a second context that shares its constants."""
    ctx2 = L.Context(0)
    m = L.Model(ctx, data, None, 1)
    r = None
    try:
        r = m.clone(ctx2)
        outs = []
        for mm, cc in ((m, ctx), (r, ctx2)):
            for name, a in feeds.items():
                mm.bind_input(name, a.shape)
            mm.prepare()
            for name, a in feeds.items():
                DeviceTensor(cc, a.shape, a.dtype, ptr=mm.input_ptrs[name], keepalive=mm).upload(a)
            cc.sync()
            for _ in range(2):
                mm.run(inputs_written_on_caller_stream=True)
                mm.sync()
            assert mm.output_dtype(0) == np.dtype(out_dtype).name
            ptr, shape = mm.output(0)
            outs.append(DeviceTensor(cc, shape, out_dtype, ptr=ptr, keepalive=mm).numpy())
        assert r.weight_arena() == m.weight_arena()  # one set of (folded) constants
        return outs
    finally:
        if r is not None:
            r.close()
        m.close()
        ctx2.close()


def every_path(ctx, tmp_path, data, feeds, out_name, want, sizes):
    """--no-fuse against the composition of rules and oracle; fused, captured, the C-ABI model and its replica against that."""
    dt = want.dtype
    unfused, _ = cli_run(tmp_path, data, feeds, out_name, dt, "--no-fuse", sizes=sizes)
    bits_equal(unfused.reshape(want.shape), want, "--no-fuse vs the composition of rules and oracle")
    fused, report = cli_run(tmp_path, data, feeds, out_name, dt, "-t", sizes=sizes)
    bits_equal(fused.reshape(want.shape), want, "fused")
    captured, rep2 = cli_run(tmp_path, data, feeds, out_name, dt, "--graph", "-n", "2", sizes=sizes)
    assert "Captured the plan into a hipGraph" in rep2
    bits_equal(captured.reshape(want.shape), want, "--graph")
    for what, got in zip(("model", "replica"), model_outputs(ctx, data, feeds, dt)):
        bits_equal(got.reshape(want.shape), want, what)
    return step_kinds(report)


def cnn_expected(q, x, quantized_output=False):
    u8 = lambda v: np.array(v, np.uint8)
    rt = lambda name, t: Q.quantize_dequantize(t, np.array(q["act"][name][0], F), u8(q["act"][name][1]))
    weight = lambda n: Q.dequantize_linear(q["weight"][n][0], q["weight"][n][1], q["weight"][n][2], axis=q["weight"][n][3])
    bias = lambda n: Q.dequantize_linear(q["bias"][n][0], q["bias"][n][1], None, axis=0)
    conv = lambda t, n, **kw: ref.conv2d_f32(t, weight(n + ".w"), bias(n + ".b"), pads=(1, 1, 1, 1), **kw)
    a = rt("a", conv(rt("x", x), "stem", strides=(2, 2), relu=True))
    b = rt("b", conv(a, "b1", relu=True))
    s = rt("s", conv(b, "b2", residual=a, relu=True))
    d = rt("d", conv(s, "dw", groups=8))
    p = rt("p", ref.max_pool(d, (2, 2), (2, 2)))
    g = rt("g", ref.global_average_pool(p).reshape(x.shape[0], 8, 1, 1)).reshape(x.shape[0], 8)
    fw, fb = weight("fc.w"), bias("fc.b")
    logits = ref.gemm_f32(g, fw.T, c=np.broadcast_to(fb, (x.shape[0], fw.shape[0])).astype(F), alpha=1.0, beta=1.0)
    scale, zp = np.array(q["act"]["logits"][0], F), u8(q["act"]["logits"][1])
    return Q.quantize_linear(logits, scale, zp) if quantized_output else Q.quantize_dequantize(logits, scale, zp)


def test_small_cnn_qdq_on_every_path(ctx, tmp_path):
    from rten_amd import onnx_writer as ow
    data, q = ow.small_cnn_qdq()
    x = np.random.default_rng(3).normal(0, 1.2, (2, 3, 16, 16)).astype(F)  # (wider than the calibration data: some values saturate)
    want = cnn_expected(q, x)
    assert len(np.unique(want)) > 5
    kinds = every_path(ctx, tmp_path, data, {"x": x}, "logits.dq", want, {"batch": 2})
    # one step per Q/DQ pair, and the f32 network's own steps around them: the folded weights are constants to every fusion
    assert kinds["QuantizeLinear+DequantizeLinear"] == q["pairs"] == 8 and kinds["QuantizeLinear"] == 0 and kinds["DequantizeLinear"] == 0, kinds
    assert kinds["Conv+Relu"] == 2 and kinds["Conv+Add+Relu"] == 1 and kinds["Conv"] == 1 and kinds["Gemm"] == 1 and kinds["MaxPool"] == 1, kinds
    assert kinds["Relu"] == 0 and kinds["Add"] == 0, kinds


def test_small_cnn_qdq_with_quantised_logits_returns_u8(ctx, tmp_path):
    from rten_amd import onnx_writer as ow
    data, q = ow.small_cnn_qdq(quantized_output=True)
    x = np.random.default_rng(4).normal(0, 1.2, (2, 3, 16, 16)).astype(F)
    want = cnn_expected(q, x, quantized_output=True)
    assert want.dtype == np.uint8 and want.shape == (2, 5)
    kinds = every_path(ctx, tmp_path, data, {"x": x}, "logits.q", want, {"batch": 2})
    assert kinds["QuantizeLinear+DequantizeLinear"] == 7 and kinds["QuantizeLinear"] == 1, kinds


def encoder_expected(cfg, w, q, ids, mask, tts):
    """oracle.models.bert_forward with the Q/DQ round trips on the inputs of the weight MatMuls and the dequantised weights."""
    B, S = ids.shape
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh
    rt = lambda name, t: Q.quantize_dequantize(t, np.array(q["act"][name][0], F), np.array(q["act"][name][1], np.uint8))

    def weight(n):
        wq, ws, wz, axis = q["weight"][n]
        return Q.dequantize_linear(wq, np.asarray(ws, F), np.asarray(wz, np.int8), axis=1 if axis is None else axis)

    m = ((F(1.0) - np.asarray(mask, F)) * np.finfo(F).min).reshape(B, 1, 1, S).astype(F)
    x = ref.add(w["word"][ids.reshape(-1)], w["type"][tts.reshape(-1)])
    x = ref.add(x, w["pos"][:S])
    x = ref.layer_norm(x, w["emb_ln_g"], w["emb_ln_b"], eps=cfg.eps)
    scale = float(F(1.0) / np.sqrt(F(dh)))
    for i, lw in enumerate(w["layers"]):
        p = f"l{i}."
        xq = rt("x0" if i == 0 else f"l{i - 1}.x2", x)
        heads = lambda t: ref.matmul_f32(xq, weight(p + "w" + t), bias=lw["b" + t]).reshape(B, S, nh, dh).transpose(0, 2, 1, 3)
        att = ref.sdpa(heads("q"), heads("k"), heads("v"), mask=m, scale=scale, flush_nan=False)
        att = np.ascontiguousarray(att.transpose(0, 2, 1, 3)).reshape(B * S, H)
        y = ref.add(ref.matmul_f32(rt(p + "ctx", att), weight(p + "wo"), bias=lw["bo"]), x)
        x = ref.layer_norm(y, lw["ln1_g"], lw["ln1_b"], eps=cfg.eps)
        h = ref.gelu(ref.matmul_f32(rt(p + "x1", x), weight(p + "w1"), bias=lw["b1"]))
        y = ref.add(ref.matmul_f32(rt(p + "h", h), weight(p + "w2"), bias=lw["b2"]), x)
        x = ref.layer_norm(y, lw["ln2_g"], lw["ln2_b"], eps=cfg.eps)
    return x.reshape(B, S, H)


def test_encoder_qdq_on_every_path(ctx, tmp_path):
    from rten_amd import onnx_writer as ow
    cfg, w, data, q = encoder_qdq()
    B, S = 2, 8
    rng = np.random.default_rng(6)
    ids = rng.integers(0, cfg.vocab, (B, S)).astype(np.int32)
    tts = rng.integers(0, 2, (B, S)).astype(np.int32)
    mask = np.ones((B, S), np.int32)
    mask[1, 5:] = 0
    want = encoder_expected(cfg, w, q, ids, mask, tts)
    feeds = {"input_ids": ids, "token_type_ids": tts, "attention_mask": mask}
    kinds = every_path(ctx, tmp_path, data, feeds, "last_hidden_state", want, {"batch": B})
    # the f32 encoder's plan plus one step per pair: the merged QKV projection, the fused attention and the MatMul epilogues all survive
    _, f32_report = cli_run(tmp_path, ow.bert_encoder(cfg, w, S), feeds, "last_hidden_state", F, "-t", sizes={"batch": B})
    f32_kinds = step_kinds(f32_report)
    assert kinds == f32_kinds + collections.Counter({"QuantizeLinear+DequantizeLinear": q["pairs"]}), (kinds, f32_kinds)
    assert any(k.startswith("MultiHeadSdpa") for k in kinds) and any(k.startswith("FusedMatMul") for k in kinds), kinds


def test_a_per_axis_step_on_dim0_refuses_sub_batch_chains(ctx):
    """Sub-batch chains split dim 0: quantisation parameters per slice of dim 0 couple the rows (axis 0 is known at load, axis -2 of a rank-2 input
    when the probe run of prepare() resolves it); per-tensor parameters and another axis do not."""
    from rten_amd import onnx_writer as ow

    def model(axis, n_scale):
        inits = [ow.tensor("s", np.full(n_scale, 0.5, F) if n_scale else np.array(0.5, F)), ow.tensor("z", np.full(n_scale, 3, np.uint8) if n_scale else np.array(3, np.uint8))]
        nodes = [ow.node("Relu", ["x"], ["r"], name="relu"), ow.node("QuantizeLinear", ["r", "s", "z"], ["q"], name="qn", axis=axis),
                 ow.node("DequantizeLinear", ["q", "s", "z"], ["y"], name="dn", axis=axis)]
        return ow.model(nodes, [ow.value_info("x", ow.FLOAT, ["batch", 4])], [ow.value_info("y", ow.FLOAT, ["batch", 4])], inits, opset=21)

    def prepare(data):
        m = L.Model(ctx, data, None, 2)
        try:
            m.bind_input("x", (4, 4))
            m.prepare()
        finally:
            m.close()

    prepare(model(0, 0))   # per-tensor: the axis does not matter
    prepare(model(1, 4))   # per column
    # (two chains of a batch of 4 run 2 rows each: the probe run of prepare() sees a 2-row tensor, so the run-time case carries 2 parameters)
    for axis, n_scale in ((0, 4), (0, 2), (-2, 2)):
        with pytest.raises(L.HipError) as e:
            prepare(model(axis, n_scale))
        assert "QuantizeLinear" in str(e.value) and '"qn"' in str(e.value) and "couples the rows" in str(e.value), str(e.value)
