"""Pad, Pow, the unary math operators, PRelu and the variadic Min / Max / Sum / Mean on the device against tests/math_rules.py: the C ABI and the
Python host operators, then PyTorch-exported graphs through the resident executor -- which runs the C++ host operators of include/rten_hip_ops.hpp --
unfused, fused and captured into a hipGraph.  Exactly specified operators are compared bit for bit (any NaN equals any NaN); Log, Softplus and Pow's
general case are held to the float64 function rounded once: within one ulp everywhere, specials exact, at most 1 element in 1000 different at all."""
import os
import sys

import numpy as np
import pytest

from oracle import ref
from rten_amd import lib as L
from rten_amd import ops
from rten_amd.tensor import DeviceTensor
from tests import math_rules as R
from tests.test_math_pad_ops import libm_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
EXACT = ["Neg", "Abs", "Sign", "Floor", "Ceil", "Round", "Sqrt", "Reciprocal", "Exp"]
CODES = {"Neg": L.UNARY_NEG, "Abs": L.UNARY_ABS, "Sign": L.UNARY_SIGN, "Floor": L.UNARY_FLOOR, "Ceil": L.UNARY_CEIL, "Round": L.UNARY_ROUND,
         "Sqrt": L.UNARY_SQRT, "Reciprocal": L.UNARY_RECIPROCAL, "Exp": L.UNARY_EXP, "Log": L.UNARY_LOG, "Softplus": L.UNARY_SOFTPLUS}
SIZES = [1, 3, 4, 5, 255, 256, 257, 4099]


def bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = got.view(np.int32) == want.view(np.int32)
    if got.dtype == np.float32:
        same |= np.isnan(got) & np.isnan(want)
    if not same.all():
        at = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {(~same).sum()} of {same.size} values differ, first at {at}: {got[at]!r} vs {want[at]!r}")


def float64_contract(got, want, what):
    """Within one ulp everywhere, non-finite values and zeros exact, at most 1 element in 1000 different at all."""
    d = R.ulp_distance(got, want)
    special = ~np.isfinite(want) | (want == 0) | (want == 1)
    frac = float((d > 0).mean())
    print(f"{what}: {int((d > 0).sum())} of {d.size} differ from the rules ({frac:.2e}), largest distance {int(d.max())} ulp")
    assert d.max() <= 1, what
    assert (d[special] == 0).all() and (np.signbit(got[special]) == np.signbit(want[special]))[~np.isnan(want[special])].all(), what
    assert (d > 0).sum() * 1000 <= d.size, what


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, 2.9387359e-39, 8.5e37, 88.7, -88.7,
                     88.73, -104.0, 104.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, -0.4, 0.4, 8388607.5, -8388608.5, 1.0, -1.0, -4.0, 9.0, 2.0, 3.0], np.float32)


def unary_inputs(n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 4).astype(np.float32)
    if n >= SPECIALS.size:
        x[:SPECIALS.size] = SPECIALS
        x[-SPECIALS.size:] = SPECIALS[::-1]  # the tail elements too
    else:
        x[:] = SPECIALS[3 * n:4 * n] if 4 * n <= SPECIALS.size else SPECIALS[:n]
    return x


_WANT = {}


def unary_want(name, n):
    """The rules' value per (operator, size), computed once."""
    if (name, n) not in _WANT:
        _WANT[name, n] = R.UNARY[name](unary_inputs(n))
    return _WANT[name, n]


def run_unary(ctx, name, x, in_place=False, offset=0):
    """offset: elements by which both pointers are moved from their allocations (the unaligned path)."""
    buf = DeviceTensor.from_numpy(ctx, np.concatenate([np.zeros(offset, np.float32), x]))
    xd = DeviceTensor(ctx, x.shape, np.float32, ptr=buf.ptr + 4 * offset, keepalive=buf)
    if in_place:
        yd, out = xd, None
    else:
        out = DeviceTensor.from_numpy(ctx, np.full(x.size + offset + 1, 7.0, np.float32))
        yd = DeviceTensor(ctx, x.shape, np.float32, ptr=out.ptr + 4 * offset, keepalive=out)
    ctx.call("rten_hip_unary_f32", CODES[name], x.size, xd.vp, yd.vp)
    ctx.sync()
    y = yd.numpy()
    if out is not None:
        guard = out.numpy()
        assert (guard[:offset] == 7.0).all() and guard[-1] == 7.0, "wrote outside y"
    return y


# ---------------------------------------------------------------------------------------------- unary
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", EXACT)
def test_exact_unary_operators_give_the_bits_of_the_rules(ctx, name, n):
    """n: 1 / 3 scalar only, 4 one vector, 5 vector + tail, 255..257 around one workgroup, 4099 several workgroups + odd tail."""
    x = unary_inputs(n)
    want = unary_want(name, n)
    bits_equal(run_unary(ctx, name, x), want, f"{name} n {n}")
    bits_equal(run_unary(ctx, name, x, in_place=True), want, f"{name} n {n} in place")
    if name == "Exp":
        bits_equal(want, ref.exp(x), "the rules' Exp is the oracle's")


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("name", EXACT + ["Log", "Softplus"])
def test_unary_operators_on_views_at_an_element_offset(ctx, name, offset):
    """Both pointers `offset` elements past a 16-byte boundary: a scalar head up to the next boundary, vectors, a scalar tail; nothing written outside."""
    for n in (2, 257):
        x = unary_inputs(n)
        want = unary_want(name, n)
        if name in EXACT:
            bits_equal(run_unary(ctx, name, x, offset=offset), want, f"{name} offset {offset}")
            bits_equal(run_unary(ctx, name, x, in_place=True, offset=offset), want, f"{name} offset {offset} in place")
        else:
            assert R.ulp_distance(run_unary(ctx, name, x, offset=offset), want).max() <= 1


def test_unary_with_differently_aligned_pointers_takes_the_scalar_path(ctx):
    x = unary_inputs(257)
    buf = DeviceTensor.from_numpy(ctx, np.concatenate([np.zeros(1, np.float32), x]))
    xd = DeviceTensor(ctx, x.shape, np.float32, ptr=buf.ptr + 4, keepalive=buf)
    yd = DeviceTensor(ctx, x.shape, np.float32)
    ctx.call("rten_hip_unary_f32", L.UNARY_SQRT, x.size, xd.vp, yd.vp)
    ctx.sync()
    bits_equal(yd.numpy(), unary_want("Sqrt", 257), "x offset, y aligned")


@pytest.mark.parametrize("name", ["Log", "Softplus"])
def test_float64_defined_unary_operators_meet_the_contract(ctx, name):
    log_x, _, _, sp_x = libm_inputs()
    x = log_x if name == "Log" else sp_x
    float64_contract(run_unary(ctx, name, x), R.UNARY[name](x), f"{name}, 4099 seeded values")
    for n in SIZES:
        xs = unary_inputs(n)
        got, want = run_unary(ctx, name, xs), unary_want(name, n)
        d = R.ulp_distance(got, want)
        special = ~np.isfinite(want) | (want == 0)
        assert d.max() <= 1 and (d[special] == 0).all(), (name, n)
        bits_equal(run_unary(ctx, name, xs, in_place=True), got, f"{name} n {n} in place")


def test_python_unary_operators_and_int32_forms(ctx):
    x = unary_inputs(257).reshape(1, 257)
    for name in EXACT:
        bits_equal(getattr(ops, name)().run(ctx, [DeviceTensor.from_numpy(ctx, x)])[0].numpy(), unary_want(name, 257).reshape(1, 257), name)
    i = np.array([I32_MIN, I32_MAX, -7, 0, 5, -1, 1, I32_MIN + 1], np.int32).reshape(2, 4)
    for name, rule in (("Neg", R.neg), ("Abs", R.abs_), ("Sign", R.sign)):
        bits_equal(getattr(ops, name)().run(ctx, [DeviceTensor.from_numpy(ctx, i)])[0].numpy(), rule(i), f"int32 {name}")
    with pytest.raises(L.HipError):
        ctx.call("rten_hip_unary_f32", 11, 4, DeviceTensor(ctx, (4,)).vp, DeviceTensor(ctx, (4,)).vp)


# ---------------------------------------------------------------------------------------------- binary and variadic
PAIRS = [((2, 3, 4, 5), ()), ((2, 3, 4, 5), (5,)), ((2, 3, 4, 5), (3, 1, 1)), ((1, 4, 1), (3, 1, 5)), ((2, 1, 3, 1, 2, 1), (1, 3, 1, 2, 1, 4)), ((2, 3, 4, 5), (2, 3, 4, 5))]


def binary_operand(shape, seed):
    """Small integers and halves (ties between the operands are frequent), both zeros, NaN."""
    rng = np.random.default_rng(seed)
    v = (rng.integers(-4, 5, int(np.prod(shape, dtype=np.int64))) * 0.5).astype(np.float32)
    if v.size >= 6:
        v[[0, 1, 2]] = [0.0, -0.0, np.nan]
        v[-3:] = [-0.0, 0.0, -2.0]
    return v.reshape(shape)


def dev(ctx, a):
    return DeviceTensor.from_numpy(ctx, a)


@pytest.mark.parametrize("pair", range(len(PAIRS)))
@pytest.mark.parametrize("name", ["Min", "Max", "Pow", "PRelu"])
def test_binary_operators_broadcast_in_both_orders(ctx, name, pair):
    sa, sb = PAIRS[pair]
    a, b = binary_operand(sa, 1 + pair), binary_operand(sb, 50 + pair)
    rule = {"Min": R.min2, "Max": R.max2, "Pow": R.pow_, "PRelu": R.prelu}[name]
    for x, y in ((a, b), (b, a)):
        if name == "PRelu" and np.broadcast_shapes(x.shape, y.shape) != x.shape:
            with pytest.raises(ops.OpError):
                ops.PRelu().run(ctx, [dev(ctx, x), dev(ctx, y)])
            continue
        if name == "Pow":
            y = np.where(np.isnan(y), F(2), y).astype(np.float32)  # (the cross table below has the NaN exponents)
        got = getattr(ops, name)().run(ctx, [dev(ctx, x), dev(ctx, y)])[0].numpy()
        want = rule(x, y)
        if name == "Pow":
            exact = np.broadcast_to((y == 2) | (y == 3), want.shape)
            bits_equal(got[exact], want[exact], f"Pow exponent 2 / 3 {x.shape} x {y.shape}")
            d = R.ulp_distance(got, want)
            special = ~np.isfinite(want) | (want == 0) | (want == 1)
            assert d.max() <= 1 and (d[special] == 0).all(), (x.shape, y.shape)
        else:
            bits_equal(got, want, f"{name} {x.shape} x {y.shape}")


def test_pow_exponent_tested_per_element_and_the_seeded_general_case(ctx):
    base = np.array([1.5, -1.5, 3.0, 0.1, 7.0, -2.0, 1e20, 1e-20, 0.3, 2.0], np.float32)
    expo = np.array([2, 3, 0.5, -1, 0, 2, 3, 0.5, -1, 0], np.float32)
    got = ops.Pow().run(ctx, [dev(ctx, base), dev(ctx, expo)])[0].numpy()
    want = R.pow_(base, expo)
    sel = (expo == 2) | (expo == 3) | (expo == 0)
    bits_equal(got[sel], want[sel], "exponents 2, 3, 0")
    assert R.ulp_distance(got, want).max() <= 1
    _, pow_b, pow_e, _ = libm_inputs()
    float64_contract(ops.Pow().run(ctx, [dev(ctx, pow_b), dev(ctx, pow_e)])[0].numpy(), R.pow_(pow_b, pow_e), "Pow, 4099 seeded pairs")
    for e in (2.0, 3.0):  # a scalar exponent: the flat kernel
        bits_equal(ops.Pow().run(ctx, [dev(ctx, pow_b), dev(ctx, np.array(e, np.float32))])[0].numpy(), R.pow_(pow_b, F(e)), f"Pow scalar {e}")
    float64_contract(ops.Pow().run(ctx, [dev(ctx, pow_b), dev(ctx, np.array(0.5, np.float32))])[0].numpy(), R.pow_(pow_b, F(0.5)), "Pow scalar 0.5")


def test_pow_special_value_cross_table(ctx):
    inf, nan = np.inf, np.nan
    base = np.array([-2, -0.0, 0.0, 0.5, 1, 2, inf, nan], np.float32)
    expo = np.array([-inf, -1, -0.5, 0, 0.5, 2, 3, inf, nan], np.float32)
    got = ops.Pow().run(ctx, [dev(ctx, base.reshape(-1, 1)), dev(ctx, expo.reshape(1, -1))])[0].numpy()
    want = R.pow_(base.reshape(-1, 1), expo.reshape(1, -1))
    bits_equal(got, want, "Pow special values (every entry of the table is exact in float64)")
    assert want[4, 8] == 1 and want[0, 4] != want[0, 4] and (want[:7, 3] == 1).all()  # pow(1, NaN) = 1, pow(-2, 0.5) = NaN, pow(x, 0) = 1


def test_int32_min_max_sum_with_the_extremes(ctx):
    a = np.array([[I32_MIN, I32_MAX, -7, 0], [5, -1, I32_MAX, I32_MIN]], np.int32)
    b = np.array([1, -1, I32_MIN, I32_MAX], np.int32)
    for name, rule in (("Min", R.vmin), ("Max", R.vmax), ("Sum", R.vsum)):
        for x, y in ((a, b), (b, a)):
            bits_equal(getattr(ops, name)().run(ctx, [dev(ctx, x), dev(ctx, y)])[0].numpy(), rule(x, y), f"int32 {name}")
    bits_equal(ops.Sum().run(ctx, [dev(ctx, a), dev(ctx, b), dev(ctx, a)])[0].numpy(), R.vsum(a, b, a), "int32 Sum of three")


def test_variadic_operators_fold_from_the_left(ctx):
    a, b, c = binary_operand((2, 1, 5), 3), binary_operand((3, 1), 4), binary_operand((5,), 5)
    big = np.array([3e38, 1e-3, 1.0, -3e38, 16777216.0], np.float32)
    for name, rule in (("Min", R.vmin), ("Max", R.vmax), ("Sum", R.vsum), ("Mean", R.mean)):
        for ins in ((a, b, c), (c, b, a), (big, big, -big), (a,)):
            got = getattr(ops, name)().run(ctx, [dev(ctx, t) for t in ins])[0].numpy()
            bits_equal(got, rule(*ins), f"{name} of {len(ins)}")
    m = np.array([1.0, 5.0, 1e-45, 3.4e38], np.float32)
    bits_equal(ops.Mean().run(ctx, [dev(ctx, m), dev(ctx, m), dev(ctx, m)])[0].numpy(), R.mean(m, m, m), "Mean divides by 3")


# ---------------------------------------------------------------------------------------------- Pad
MODES = ["constant", "reflect", "edge", "wrap"]
HW = [(1, 1), (3, 4), (5, 7), (4, 16), (2, 33)]


def run_pad(ctx, x, pads, mode, value=None):
    inputs = [dev(ctx, x), np.asarray(pads, np.int32)]
    if value is not None:
        inputs.append(dev(ctx, np.asarray(value, x.dtype)))
    return ops.Pad(mode).run(ctx, inputs)[0].numpy()


def pad_amounts(length, mode):
    return [0, 1, 2, length - 1, length, length + 2] if mode in ("reflect", "wrap") else [0, 1, 2, length - 1]


_PAD_X = {}


def pad_input(h, w):
    if (h, w) not in _PAD_X:
        _PAD_X[h, w] = np.arange(2 * 3 * h * w, dtype=np.float32).reshape(2, 3, h, w) + F(0.25)
    return _PAD_X[h, w]


@pytest.mark.parametrize("hw", HW)
@pytest.mark.parametrize("mode", MODES)
def test_pad_every_mode_and_amount_gives_the_rules(ctx, mode, hw):
    """Every amount on one side of one axis with a fixed amount elsewhere, then seeded combinations of all four sides: (4, 16) with an unpadded W takes
    the 16-byte path, every other case the 4-byte one."""
    h, w = hw
    x = pad_input(h, w)
    cases = []
    for p in pad_amounts(h, mode):
        cases += [(p, 1, 0, 2), (1, 0, p, 0)]
    for p in pad_amounts(w, mode):
        cases += [(1, p, 2, 0), (0, 0, 1, p)]
    rng = np.random.default_rng(h * 100 + w)
    ah, aw = pad_amounts(h, mode), pad_amounts(w, mode)
    cases += [(int(rng.choice(ah)), int(rng.choice(aw)), int(rng.choice(ah)), int(rng.choice(aw))) for _ in range(6)]
    for t, l, b, r in cases:
        pads = [0, 0, t, l, 0, 0, b, r]
        if (t, l, b, r) == (0, 0, 0, 0):
            continue
        bits_equal(run_pad(ctx, x, pads, mode, F(-1.5) if mode == "constant" else None), R.pad(x, pads, mode, F(-1.5)), f"{mode} {hw} pads {pads}")


@pytest.mark.parametrize("mode", MODES)
def test_pad_mixed_negative_and_positive_entries(ctx, mode):
    for h, w in ((5, 7), (4, 16)):
        x = pad_input(h, w)
        for pads in ([0, 0, -1, 2, 0, 0, 1, -3], [0, 0, 2, -4, 0, 0, -2, 3], [0, 0, -2, 0, 0, 0, 3, 0], [0, 0, -1, -1, 0, 0, -1, -1], [-1, 0, 1, 1, 0, -2, 1, 1],
                     [0, 0, 0, -4, 0, 0, 2, 0]):
            bits_equal(run_pad(ctx, x, pads, mode), R.pad(x, pads, mode), f"{mode} {(h, w)} pads {pads}")


def test_pad_constant_on_every_axis_of_1d_and_6d_tensors(ctx):
    x1 = np.arange(1, 8, dtype=np.float32)
    for pads in ([2, 3], [-2, 1], [0, 5]):
        bits_equal(run_pad(ctx, x1, pads, "constant", F(9)), R.pad(x1, pads, "constant", F(9)), f"1-D {pads}")
    for mode in MODES[1:]:
        bits_equal(run_pad(ctx, x1, [9, 8], mode), R.pad(x1, [9, 8], mode), f"1-D {mode}: one row")
    x6 = np.arange(2 * 3 * 2 * 3 * 2 * 5, dtype=np.float32).reshape(2, 3, 2, 3, 2, 5)
    pads = [1, 0, 2, -1, 1, 2, 0, 1, -1, 1, 0, 1]
    bits_equal(run_pad(ctx, x6, pads, "constant", F(-0.0)), R.pad(x6, pads, "constant", F(-0.0)), "6-D, every axis")
    bits_equal(run_pad(ctx, x6, [1] * 12, "constant"), R.pad(x6, [1] * 12, "constant"), "6-D, default fill")


def test_pad_int32_fill_identity_and_empty_outputs(ctx):
    xi = (np.arange(2 * 3 * 4 * 4, dtype=np.int32).reshape(2, 3, 4, 4) - 40) * 1000003
    for pads in ([0, 1, 2, 0, 1, 0, 0, 3], [1, 0, 0, 0, 0, 0, 2, 0]):
        bits_equal(run_pad(ctx, xi, pads, "constant", np.int32(I32_MIN + 5)), R.pad(xi, pads, "constant", np.int32(I32_MIN + 5)), f"int32 {pads}")
    bits_equal(run_pad(ctx, xi, [0, 0, 1, 1, 0, 0, 1, 1], "reflect"), R.pad(xi, [0, 0, 1, 1, 0, 0, 1, 1], "reflect"), "int32 reflect")
    x = pad_input(3, 4)
    for mode in MODES:
        bits_equal(run_pad(ctx, x, [0] * 8, mode), x, f"identity {mode}")
        y = run_pad(ctx, x, [0, 0, -1, 0, 0, 0, -2, 0], mode)  # cropped to nothing: the empty crop is the result in every mode
        assert y.shape == (2, 3, 0, 4) and y.dtype == np.float32
    y = run_pad(ctx, x, [0, 0, -1, 0, 0, 0, -2, 1], "constant")
    assert y.shape == (2, 3, 0, 5)
    with pytest.raises(ops.OpError):
        run_pad(ctx, x, [0, 0, -1, 0, 0, 0, -2, 1], "reflect")
    y = run_pad(ctx, np.zeros((2, 0, 3), np.float32), [0, 2, 0, 0, 0, 1], "constant", F(4))
    bits_equal(y, np.full((2, 2, 4), 4, np.float32), "an empty input: every element is the fill")
    with pytest.raises(L.HipError):  # the entry point's own checks
        ctx.call("rten_hip_pad_b32", L.PAD_REFLECT, 2, ops._i64([3, 0]), ops._i64([0, 2, 0, 0]), 0, None, DeviceTensor(ctx, (3, 2)).vp)
    with pytest.raises(L.HipError):
        ctx.call("rten_hip_pad_b32", L.PAD_CONSTANT, 1, ops._i64([3]), ops._i64([-2, -2]), 0, DeviceTensor(ctx, (3,)).vp, DeviceTensor(ctx, (3,)).vp)
    with pytest.raises(L.HipError):
        ctx.call("rten_hip_pad_b32", 4, 1, ops._i64([3]), ops._i64([1, 1]), 0, DeviceTensor(ctx, (3,)).vp, DeviceTensor(ctx, (5,)).vp)


# ---------------------------------------------------------------------------------------------- exported graphs through the resident executor
def _te():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export as te
    return te


GRAPH_MODES = (("--no-fuse",), (), ("--graph", "-n", "3"))


def run_graph(tmp_path, data, inputs, out_name, *flags, sizes=None):
    """One rten_hip_run process: `inputs` = {name: float32 array}; returns the flat output and the tool's report."""
    from tests.test_graph_executor import run_cli
    model, yout = tmp_path / "m.onnx", tmp_path / "y.bin"
    model.write_bytes(data)
    args = []
    for name, a in inputs.items():
        f = tmp_path / f"{name}.bin"
        f.write_bytes(np.ascontiguousarray(a, np.float32).tobytes())
        args += ["--input", f"{name}={f}"]
    for k, v in (sizes or {}).items():
        args += ["-s", f"{k}={v}"]
    out = run_cli(*flags, *args, "--dump", f"{out_name}={yout}", str(model))
    assert out.returncode == 0, out.stderr + out.stdout
    return np.fromfile(yout, np.float32), out.stdout


def three_ways(tmp_path, data, inputs, out_name, want, sizes=None):
    """Unfused against the composition of oracle / rules functions, then fused and captured against unfused: all bit for bit."""
    runs = [run_graph(tmp_path, data, inputs, out_name, *flags, sizes=sizes) for flags in GRAPH_MODES]
    assert "Captured the plan into a hipGraph" in runs[2][1]
    got = [r[0].reshape(want.shape) for r in runs]
    bits_equal(got[0], want, "--no-fuse vs the composition of oracle / rules functions")
    bits_equal(got[1], got[0], "fused vs --no-fuse")
    bits_equal(got[2], got[0], "--graph vs --no-fuse")
    return got[1]


def reflect_generator_expected(module, x):
    from tests import norm_rules as N
    p = {k: v.detach().numpy() for k, v in module.state_dict().items()}
    inorm = lambda t, k: N.instance_norm(t, p[k + ".weight"], p[k + ".bias"], 1e-5)
    conv = lambda t, k: ref.conv2d_f32(t, p[k + ".weight"], p[k + ".bias"])
    prelu = lambda t, k: R.prelu(t, p[k + ".weight"].reshape(-1, 1, 1))
    pad2 = lambda t, n, mode: R.pad(t, [0, 0, n, n, 0, 0, n, n], mode)
    y = prelu(inorm(conv(pad2(x, 3, "reflect"), "stem.1"), "stem.2"), "stem.3")
    for b in ("blocks.0.body.", "blocks.1.body."):
        t = prelu(inorm(conv(pad2(y, 1, "reflect"), b + "1"), b + "2"), b + "3")
        y = ref.add(y, inorm(conv(pad2(t, 1, "reflect"), b + "5"), b + "6")).reshape(y.shape)
    y = R.pad(y, [0, 0, -1, 1, 0, 0, 2, -2], "constant")  # F.pad(y, (1, -2, -1, 2))
    return ref.tanh(conv(pad2(y, 1, "edge"), "out.1"))


def test_exported_reflect_generator(tmp_path):
    import torch
    te = _te()
    module = te.reflect_generator_module(seed=5)
    data = te.reflect_generator_onnx(module, dynamic=True)
    x = (np.random.default_rng(2).random((2, 3, 16, 16), dtype=np.float32) - F(0.5)).astype(np.float32)
    got = three_ways(tmp_path, data, {"x": x}, "y", reflect_generator_expected(module, x), sizes={"batch": 2})
    with torch.no_grad():
        t = module(torch.from_numpy(x)).numpy()
    diff = np.abs(got - t).max()
    print(f"reflect_generator: max |device - torch| = {diff:.3e}")
    assert got.shape == t.shape and diff <= 1e-4  # expect_eq_1e4: the reference's bar for these operators


def gpt2_mlp_expected(module, x):
    p = {k: v.detach().numpy() for k, v in module.state_dict().items()}
    rows = x.reshape(-1, x.shape[-1])
    h = ref.layer_norm(rows, p["ln.weight"], p["ln.bias"], eps=1e-5)
    h = (p["fc.bias"] + ref.matmul_f32(h, np.ascontiguousarray(p["fc.weight"].T))).astype(np.float32)
    half = (h * F(0.5)).astype(np.float32)
    inner = (h + (R.pow_(h, F(3.0)) * F(0.044715)).astype(np.float32)).astype(np.float32)
    gate = (ref.tanh((inner * F(0.7978845608028654)).astype(np.float32)) + F(1.0)).astype(np.float32)
    act = (half * gate).astype(np.float32)
    y = (p["proj.bias"] + ref.matmul_f32(act, np.ascontiguousarray(p["proj.weight"].T))).astype(np.float32)
    return y.reshape(x.shape[0], x.shape[1], -1)


def test_exported_gpt2_mlp(tmp_path):
    te = _te()
    module = te.gpt2_mlp_module(seed=6)
    data = te.gpt2_mlp_onnx(module, dynamic=True)
    for batch in (2, 3):
        x = (np.random.default_rng(batch).standard_normal((batch, 5, 32)) * 2).astype(np.float32)
        three_ways(tmp_path, data, {"x": x}, "y", gpt2_mlp_expected(module, x), sizes={"batch": batch})


def box_decode_expected(module, x, grid):
    p = {k: v.detach().numpy() for k, v in module.state_dict().items()}
    a = p["anchor_wh"].shape[1] // 2
    f = lambda v: np.asarray(v, np.float32)
    t = ref.conv2d_f32(x, p["head.weight"], p["head.bias"], pads=(1, 1, 1, 1))
    cx, cy = f(grid[:, 0:1] + t[:, 0:a]), f(grid[:, 1:2] + t[:, a:2 * a])
    wh = f(R.exp(t[:, 2 * a:]).reshape(t[:, 2 * a:].shape) * p["anchor_wh"])
    w2, h2 = f(wh[:, :a] * F(0.5)), f(wh[:, a:] * F(0.5))
    x0, y0 = R.max2(f(cx - w2), p["lo"]), R.max2(f(cy - h2), p["lo"])
    x1, y1 = R.min2(f(cx + w2), p["hi_x"]), R.min2(f(cy + h2), p["hi_y"])
    side = R.sqrt(R.abs_(f(f(x1 - x0) * f(y1 - y0))))
    inv = R.reciprocal(f(side + F(1.0)))
    return np.concatenate([x0, y0, x1, y1, side, inv, R.neg(R.abs_(t[:, 0:a]))], 1)


def test_exported_box_decoder(tmp_path):
    te = _te()
    module = te.box_decode_module(seed=7)
    data = te.box_decode_onnx(module, dynamic=True)
    gy, gx = np.meshgrid(np.arange(6, dtype=np.float32) * 8 + 4, np.arange(8, dtype=np.float32) * 8 + 4, indexing="ij")
    grid = np.stack([gx, gy])[None].astype(np.float32)
    for batch in (2, 3):
        x = (np.random.default_rng(batch).standard_normal((batch, 4, 6, 8)) * 3).astype(np.float32)  # large offsets: boxes leave the image on every side
        want = box_decode_expected(module, x, grid)
        assert (want[:, 0:3] == 0).any() and (want[:, 6:9] == 64).any()  # the clipping is exercised
        three_ways(tmp_path, data, {"x": x, "grid": grid}, "boxes", want, sizes={"batch": batch})


@pytest.mark.parametrize("scale", [2.0, 1.5])
def test_dynamic_upsample_at_two_bound_sizes(tmp_path, scale):
    """The output size is Floor(Cast(Shape) * scale) evaluated on the host (scale 1.5: the Floor matters at odd sizes); pads / constant_value of the Pad are inputs."""
    from tests.test_gpu_resize_split import np_resize
    te = _te()
    w = te.dynamic_upsample_weights(seed=8)
    data = te.dynamic_upsample_onnx(w, scale=scale)
    for n, h, wd in ((1, 6, 8), (2, 5, 7)):
        x = (np.random.default_rng(h).random((n, 3, h, wd), dtype=np.float32) - F(0.5)).astype(np.float32)
        a = ref.conv2d_f32(x, w["a.weight"], w["a.bias"], pads=(1, 1, 1, 1))
        oh, ow = int(np.floor(F(h) * F(scale))), int(np.floor(F(wd) * F(scale)))
        up = np_resize(a, sizes=[n, 4, oh, ow], mode="nearest", coord="asymmetric", nearest="floor")
        want = ref.conv2d_f32(R.pad(up, [0, 0, 1, 1, 0, 0, 1, 1], "constant", F(0.5)), w["b.weight"], w["b.bias"])
        assert want.shape == (n, 3, oh, ow)
        three_ways(tmp_path, data, {"x": x}, "y", want, sizes={"batch": n, "height": h, "width": wd})


def test_executor_refuses_device_resident_pads(tmp_path):
    from rten_amd import onnx_writer as ow
    from tests.test_graph_executor import run_cli
    # pads computed from device data (a Cast of a graph input's values): an OpError that says so, when the step runs
    nodes = [ow.node("Cast", ["p"], ["pi"], name="cast_p", to=7), ow.node("Pad", ["x", "pi"], ["y"], name="pad_node")]
    data = ow.model(nodes, [ow.value_info("x", 1, [2, 3]), ow.value_info("p", 1, [4])], [ow.value_info("y", 1, [2, 5])], [])
    model, xin, pin = tmp_path / "m.onnx", tmp_path / "x.bin", tmp_path / "p.bin"
    model.write_bytes(data)
    xin.write_bytes(np.zeros((2, 3), np.float32).tobytes())
    pin.write_bytes(np.array([0, 1, 0, 1], np.float32).tobytes())
    out = run_cli("--input", f"x={xin}", "--input", f"p={pin}", str(model))
    assert out.returncode != 0 and "Pad: pads must be a constant or computable from the input shapes" in out.stderr, out.stderr + out.stdout


def test_a_pad_of_dim0_refuses_sub_batch_chains(ctx):
    """Sub-batch chains split dim 0: a Pad that pads or crops it couples the rows (noted when the probe run of prepare() sees the pads); a spatial Pad does not."""
    from rten_amd import onnx_writer as ow

    def model(pads, out_shape):
        nodes = [ow.node("Relu", ["x"], ["r"], name="relu"), ow.node("Pad", ["r", "pads"], ["y"], name="pad_node", mode="constant")]
        return ow.model(nodes, [ow.value_info("x", 1, ["batch", 3, 4, 4])], [ow.value_info("y", 1, out_shape)], [ow.tensor("pads", np.array(pads, np.int64))])

    def prepare(data):
        m = L.Model(ctx, data, None, 2)
        try:
            m.bind_input("x", (4, 3, 4, 4))
            m.prepare()
        finally:
            m.close()

    prepare(model([0, 0, 1, 1, 0, 0, 1, 1], ["batch", 3, 6, 6]))
    with pytest.raises(L.HipError) as e:
        prepare(model([1, 0, 0, 0, 0, 0, 0, 0], ["batch2", 3, 4, 4]))
    assert 'Pad "pad_node" (pads or crops dim 0)' in str(e.value) and "couples the rows" in str(e.value), str(e.value)
