"""ReduceL1 / ReduceSumSquare / ReduceL2 / ReduceLogSum / ReduceLogSumExp / ReduceProd, LpNormalization and GlobalMaxPool without a GPU: (1) the restated
rules (tests/reduce_rules.py) against the literals of the reference's own tests (tests/golden/reduce_reference.json); (2) the float32 fused multiply-add the
SumSquare rule stands on, against exact rational arithmetic; (3) the Python operators' host logic -- shapes, keepdims, axes resolution, the stride lists
handed to the C ABI, the launch lists, every error -- on a simulated context whose entry points ARE the restatement; (4) registries, header and bindings."""
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from rten_amd import einsum as E
from rten_amd import lib, ops
from tests import reduce_rules as R
from tests import select_rules
from tests.test_select_ops import SimCtx, _row_major, dev, permuted, raises

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "reduce_reference.json")))
F = np.float32
OPS = {"l1": ops.ReduceL1, "sum_square": ops.ReduceSumSquare, "l2": ops.ReduceL2, "log_sum": ops.ReduceLogSum, "log_sum_exp": ops.ReduceLogSumExp,
       "prod": ops.ReduceProd}
KIND_CODE = {"l1": 0, "sum_square": 1, "l2": 2, "log_sum": 3, "log_sum_exp": 4, "prod": 5}


def _num(v):
    return {"-inf": -np.inf, "inf": np.inf, "nan": np.nan}.get(v, v) if isinstance(v, str) else v


# ------------------------------------------------------------------------------------------ 1. restatement vs the reference's literals
def _expected(case, x):
    """The expectation of a golden case as a float64 / int array: a literal list, or the arithmetic the reference's test states, evaluated as it does."""
    e = case.get("expected_expr")
    if e is None:
        return np.array([_num(v) for v in case["expected"]], np.float64)
    if e == "left_product":  # input.iter().product::<f32>()
        p = F(1)
        for v in x.reshape(-1):
            p = F(p * v)
        return np.array([p], np.float64)
    if e == "left_sum_of_squares":  # input.iter().map(|x| x * x).sum::<f32>()
        s = F(0)
        for v in x.reshape(-1):
            s = F(s + F(v * v))
        return np.array([s], np.float64)
    if e == "ln_of":  # 6f32.ln(), 15f32.ln()
        return np.array([np.log(F(v)) for v in case["expected_args"]], np.float64)
    if e == "add_ln":  # 100. + 2f32.ln()
        a, b = case["expected_args"]
        return np.array([F(a) + np.log(F(b))], np.float64)
    if e == "ln_sum_exp_rows":  # (exp[[r, 0]] + exp[[r, 1]] + exp[[r, 2]]).ln()
        return np.array([np.log(np.exp(r.astype(np.float32)).sum(dtype=np.float32)) for r in x], np.float64)
    raise AssertionError(e)


@pytest.mark.parametrize("i", range(len(GOLDEN["reduce"])))
def test_rules_reproduce_the_reference_literals(i):
    case = GOLDEN["reduce"][i]
    x = np.array(case["input"], case["dtype"]).reshape(case["shape"])
    got = R.reduce(case["kind"], x, case["axes"], case["keepdims"])
    assert list(got.shape) == case["expected_shape"] and got.dtype == x.dtype
    want = _expected(case, x).reshape(case["expected_shape"])
    if case["compare"] == "assert_eq":
        assert np.array_equal(got.astype(np.float64), want), (got, want)
    else:  # expect_equal: absolute 1e-5 (the reference's helper)
        assert np.allclose(got.astype(np.float64), want, rtol=0, atol=1e-5 * max(1.0, float(np.abs(want).max()))), (got, want)


def test_noop_rules_reproduce_the_reference():
    for case in GOLDEN["noop_with_empty_axes"]:
        x = np.array(case["input"], np.float32)
        want = {"x_times_x": x * x, "identity": x, None: np.array(case.get("expected", []), np.float32)}[case.get("expected_expr")]
        for axes in (None, []):
            R.same_bits(R.reduce(case["kind"], x, axes, False, noop_with_empty_axes=True), want, case["kind"])
    R.same_bits(R.reduce("log_sum", F([1.0, 0.0, -1.0, 8.0]), None, True, True), F([0.0, -np.inf, np.nan, np.log(8.0)]))  # Log(ReduceSum(x)): the log stays
    R.same_bits(R.reduce("log_sum_exp", F([1.0, -2.0]), None, True, True), F([1.0, -2.0]))                               # log(exp(x)) = x
    R.same_bits(R.reduce("l1", np.array([-3, 4, -2**31], np.int32), None, True, True), np.array([3, 4, -2**31], np.int32))
    R.same_bits(R.reduce("sum_square", np.array([-3, 65536], np.int32), None, True, True), np.array([9, 0], np.int32))


def test_lp_normalization_literals():
    for case in GOLDEN["lp_normalization"]:
        x = np.array(case["input"], np.float32).reshape(case["shape"])
        den = np.array([np.sqrt(F(2)) if d == "sqrt2" else d for d in case["expected_den"]], np.float32)
        want = (np.array(case["expected_num"], np.float32) / den).reshape(case["shape"])
        got = R.lp_normalization(x, case["axis"], case["p"])
        assert np.allclose(got, want, rtol=0, atol=1e-5), (got, want)
    e = GOLDEN["errors"]["lp_normalization_p"]
    with pytest.raises(R.RuleError) as err:
        R.lp_normalization(np.zeros((2, 2), F), 0, e["p"])
    assert (err.value.kind, err.value.msg) == (e["kind"], e["message"])
    x = F([[0.0, 0.0], [3.0, 4.0]])
    R.same_bits(R.lp_normalization(x, -1, 2), F([[0.0, 0.0], [F(3) * (F(1) / F(5)), F(4) * (F(1) / F(5))]]))  # x * (1 / norm), not x / norm
    assert R.lp_normalization(np.zeros((3, 0), F), 1, 1).shape == (3, 0)


def test_empty_slices_and_zero_d():
    for kind, ident in (("l1", 0.0), ("sum_square", 0.0), ("l2", 0.0), ("prod", 1.0), ("log_sum", -np.inf), ("log_sum_exp", -np.inf)):
        R.same_bits(R.reduce(kind, np.zeros((2, 0, 3), F), [1], False), np.full((2, 3), ident, F), kind)
        assert R.reduce(kind, np.zeros((2, 0, 3), F), [0], True).shape == (1, 0, 3)
    for kind, ident in (("l1", 0), ("sum_square", 0), ("prod", 1)):
        R.same_bits(R.reduce(kind, np.zeros((2, 0), np.int32), [1], True), np.full((2, 1), ident, np.int32), kind)
    # a 0-d input is a slice of one element (reduce.rs:430-433)
    for kind, want in (("l1", 2.5), ("sum_square", 6.25), ("l2", 2.5), ("prod", -2.5), ("log_sum", np.nan), ("log_sum_exp", -2.5)):
        R.same_bits(R.reduce(kind, F(-2.5), None, True), F(want), kind)
    with pytest.raises(R.RuleError, match="Axis is invalid"):
        R.reduce("l2", F(1.0), [0], True)


def test_int32_rules_wrap():
    big = np.array([[2**31 - 1, 1, -2**31], [65536, 65536, 3]], np.int32)
    R.same_bits(R.reduce("l1", big, [1], False), np.array([0, 131075], np.int32))                       # MAX + 1 + |MIN| (= MIN) wraps to 0
    R.same_bits(R.reduce("prod", big, [1], False), np.array([-2**31, 0], np.int32))                      # 2^32 * 3 = 0
    R.same_bits(R.reduce("sum_square", np.array([46341, 2], np.int32), [0], False), np.array(-2147479011, np.int32))
    for kind in ("l2", "log_sum", "log_sum_exp"):
        with pytest.raises(R.RuleError):
            R.reduce(kind, big, [1], False)


# ------------------------------------------------------------------------------------------ 2. fmaf is the correctly rounded fused multiply-add
def _round_to_f32(q: Fraction) -> np.float32:
    """The float32 nearest to the rational q, ties to even (finite results in the normal range only)."""
    if q == 0:
        return F(0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert -126 <= e <= 127
    scaled = a / Fraction(2) ** (e - 23)  # in [2^23, 2^24)
    n, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and n % 2):
        n += 1
    return F(sign * float(Fraction(n) * Fraction(2) ** (e - 23)))


def test_fmaf_against_exact_rational_arithmetic():
    rng = np.random.default_rng(20240611)
    differs_from_double_rounding = 0
    for _ in range(400):
        x = F(rng.standard_normal() * 10.0 ** int(rng.integers(-3, 4)))
        acc = F(abs(rng.standard_normal()) * 10.0 ** int(rng.integers(-3, 6)))
        want = _round_to_f32(Fraction(float(x)) * Fraction(float(x)) + Fraction(float(acc)))
        got = R.fmaf(x, x, acc)
        assert got.view(np.uint32) == want.view(np.uint32), (x, acc, got, want)
        differs_from_double_rounding += int(F(F(x * x) + acc).view(np.uint32) != want.view(np.uint32))
    assert differs_from_double_rounding > 0  # (otherwise the slots say nothing about the fusion)
    # one SumSquare slot chain, exactly: lane 0 of a 17-element slice holds fma(x16, x16, fma(x0, x0, 0))
    xs = rng.standard_normal(17).astype(np.float32)
    lane0 = _round_to_f32(Fraction(float(xs[16])) ** 2 + Fraction(float(_round_to_f32(Fraction(float(xs[0])) ** 2))))
    rest = [_round_to_f32(Fraction(float(v)) ** 2) for v in xs[1:16]]
    s = F(0)
    for v in [lane0] + rest:
        s = F(s + v)
    assert R.sum_square(xs).view(np.uint32) == s.view(np.uint32)


def test_sum_abs_and_sum_square_follow_the_oracle_sum_order():
    from oracle import einsum as oe
    rng = np.random.default_rng(3)
    for n in (1, 15, 16, 17, 63, 64, 65, 129, 257):
        x = rng.standard_normal(n).astype(np.float32)
        # with the plain add as the fold, the restated walk IS the oracle's Sum: the order is the shared part
        assert R.fold_unroll4(x, lambda a, v: F(a + v)).view(np.uint32) == F(oe.reduce_sum(x, [0])).view(np.uint32), n
        assert R.sum_abs(x).view(np.uint32) == R.fold_unroll4(x, lambda a, v: F(a + abs(v))).view(np.uint32), n


def test_prod_row_tells_orders_apart():
    row = prod_row()
    assert R.prod(row).view(np.uint32) != R.pairwise_prod(row).view(np.uint32)


def prod_row():
    """257 values near 1 whose left fold and pairwise product differ in at least one bit (seed chosen on the CPU; shared with the GPU test)."""
    return (1 + np.random.default_rng(7).standard_normal(257) * 1e-2).astype(np.float32)


# ------------------------------------------------------------------------------------------ 3. host logic on a simulated context
class Sim(SimCtx):
    """SimCtx plus the two new entry points (= the restatement) and the element-wise calls the noop forms make."""

    def call(self, name, *a):
        val = lambda v: int(v.value if hasattr(v, "value") else v)
        dts = {0: np.float32, 1: np.int32}
        if name == "rten_hip_reduce_strided":
            self.launches.append((name, a))
            kind, dt, no, osh, ost, ni, ish, ist, x, y = a
            assert no <= 6 and ni <= 6
            osh, ost, ish, ist = list(osh)[:no], list(ost)[:no], list(ish)[:ni], list(ist)[:ni]
            v = self._view(self._addr(x), osh + ish, ost + ist, dts[dt])
            out = self._view(self._addr(y), osh, _row_major(osh), dts[dt])
            k = R.KINDS[kind]
            if ni:
                out[...] = R.reduce(k, v, list(range(no, no + ni)), False)
            else:  # no reduced dims: every element is a slice of one
                out[...] = np.array([R.reduce(k, e, None, False) for e in np.ascontiguousarray(v).reshape(-1)], dts[dt]).reshape(v.shape)
        elif name == "rten_hip_lp_normalize_f32":
            self.launches.append((name, a))
            p, no, osh, ost, n, st, x, y = a
            osh, ost = list(osh)[:no], list(ost)[:no]
            v = self._view(self._addr(x), osh + [n], ost + [st], np.float32)
            self._view(self._addr(y), osh + [n], ost + [st], np.float32)[...] = R.lp_normalization(np.ascontiguousarray(v), -1, p)
        elif name == "rten_hip_unary_f32":
            self.launches.append((name, a))
            code, n, x, y = a
            v = self._view(self._addr(x), [val(n)], [1], np.float32)
            self._view(self._addr(y), [val(n)], [1], np.float32)[...] = R.noop_value({lib.UNARY_ABS: "l1", lib.UNARY_LOG: "log_sum"}[code], v.copy())
        elif name == "rten_hip_mul_f32":
            self.launches.append((name, a))
            n, x, b, bn, y = a
            assert val(n) == val(bn)
            v, w = self._view(self._addr(x), [val(n)], [1], np.float32), self._view(self._addr(b), [val(n)], [1], np.float32)
            self._view(self._addr(y), [val(n)], [1], np.float32)[...] = v * w
        elif name == "rten_hip_elementwise_nd":
            self.launches.append((name, a))
            op, nd, shape, x, xdt, xst, b, bdt, bst, c, cst, y, ydt = a
            assert nd == 1 and xdt == ydt == lib.DT_I32 and op in (lib.EW_IABS, lib.EW_IMUL)
            n = list(shape)[0]
            v = self._view(self._addr(x), [n], [1], np.int32)
            self._view(self._addr(y), [n], [1], np.int32)[...] = R.noop_value("l1" if op == lib.EW_IABS else "sum_square", v.copy())
        else:
            super().call(name, *a)


def rng_x(shape, seed=0, dtype=np.float32):
    r = np.random.default_rng(seed)
    return r.integers(-5, 6, size=shape).astype(dtype) if dtype == np.int32 else (r.standard_normal(shape) * 2).astype(np.float32)


@pytest.mark.parametrize("kind", R.KINDS)
def test_reduce_shapes_axes_keepdims(kind):
    c = Sim()
    cls = OPS[kind]
    dtypes = [np.float32] + ([np.int32] if kind in R.INT32_KINDS else [])
    for dtype in dtypes:
        x = rng_x((2, 3, 4, 5), 1, dtype)
        if kind == "log_sum":
            x = np.abs(x) + 1
        for axes in (None, [], [0], [3], [-1], [1, 2], [2, 1, -2], [0, 1, 2, 3], [-4, 3]):
            for keep in (True, False):
                got = cls(axes=axes, keep_dims=keep).run(c, [dev(c, x)])[0]
                R.same_bits(got.numpy(), R.reduce(kind, x, axes, keep), (kind, axes, keep))
                assert c.launches[-1][0] == "rten_hip_reduce_strided" and c.launches[-1][1][0] == KIND_CODE[kind] and c.launches[-1][1][1] == (0 if dtype == np.float32 else 1)
                # axes as the second input override the attribute
                got = cls(axes=[0], keep_dims=keep).run(c, [dev(c, x), None if axes is None else np.array(axes, np.int32)])[0]
                R.same_bits(got.numpy(), R.reduce(kind, x, [0] if axes is None else axes, keep))
        # noop_with_empty_axes: the reduction is skipped, the operator's element map is not
        n = len(c.launches)
        for op in (cls(axes=[], noop_with_empty_axes=True), cls(noop_with_empty_axes=True)):
            R.same_bits(op.run(c, [dev(c, x)])[0].numpy(), R.reduce(kind, x, None, True, True), kind)
        names = [l[0] for l in c.launches[n:]]
        expect = {"l1": "rten_hip_unary_f32" if dtype == np.float32 else "rten_hip_elementwise_nd", "log_sum": "rten_hip_unary_f32",
                  "sum_square": "rten_hip_mul_f32" if dtype == np.float32 else "rten_hip_elementwise_nd"}.get(kind)
        assert names == (["rten_hip_copy_strided_b32"] + ([expect] if expect else [])) * 2, names
        # a 0-d input is a slice of one element; naming an axis of it is an error
        s = np.array(3 if dtype == np.int32 else 1.75, dtype)
        R.same_bits(cls().run(c, [dev(c, s)])[0].numpy(), R.reduce(kind, s, None, True), kind)
        name, a = c.launches[-1]
        assert name == "rten_hip_reduce_strided" and (a[2], a[5]) == (0, 0)
        raises(lambda: cls(axes=[0]).run(c, [dev(c, s)]), ops.InvalidValue("Axis is invalid"))
        raises(lambda: cls(axes=[4]).run(c, [dev(c, x)]), ops.InvalidValue("Axis is invalid"))
        raises(lambda: cls(axes=[-5]).run(c, [dev(c, x)]), ops.InvalidValue("Axis is invalid"))
        # empty slices give the kernel's value; an empty output launches nothing
        e = np.zeros((2, 0, 3), dtype)
        R.same_bits(cls(axes=[1], keep_dims=False).run(c, [dev(c, e)])[0].numpy(), R.reduce(kind, e, [1], False), kind)
        n = len(c.launches)
        assert cls(axes=[0]).run(c, [dev(c, e)])[0].shape == (1, 0, 3) and len(c.launches) == n
    raises(lambda: cls().run(c, []), ops.MissingInputs)
    op = cls()
    assert (op.axes, op.keep_dims, op.noop_with_empty_axes, op.max_inputs(), op.name()) == (None, True, False, 2, cls.__name__)


def test_reduce_type_refusals():
    c = Sim()
    xi, xu = np.arange(6, dtype=np.int32).reshape(2, 3), np.zeros(3, np.uint8)
    cast = ops.OpError("InputCastFailed", "expected float32 tensor")
    raises(lambda: ops.ReduceL2(axes=[1]).run(c, [dev(c, xi)]), ops.UnsupportedType)  # map_value_view!(.., [FloatTensor], ..)
    raises(lambda: ops.ReduceLogSum(axes=[1]).run(c, [dev(c, xi)]), cast)             # require_as::<f32>
    raises(lambda: ops.ReduceLogSumExp(axes=[1]).run(c, [dev(c, xi)]), cast)
    raises(lambda: ops.ReduceLogSum(noop_with_empty_axes=True).run(c, [dev(c, xi)]), cast)      # ... which comes before the noop test
    raises(lambda: ops.ReduceLogSumExp(noop_with_empty_axes=True).run(c, [dev(c, xi)]), cast)
    R.same_bits(ops.ReduceL2(noop_with_empty_axes=True).run(c, [dev(c, xi)])[0].numpy(), xi)    # L2 / Prod copy before they look at the type
    R.same_bits(ops.ReduceProd(noop_with_empty_axes=True).run(c, [dev(c, xi)])[0].numpy(), xi)
    for cls in (ops.ReduceL1, ops.ReduceSumSquare, ops.ReduceProd, ops.ReduceL2):
        raises(lambda: cls(axes=[0]).run(c, [dev(c, xu)]), ops.UnsupportedType)
    for cls in (ops.ReduceL1, ops.ReduceSumSquare):
        raises(lambda: cls(noop_with_empty_axes=True).run(c, [dev(c, xu)]), ops.UnsupportedType)  # typed before the noop test


def test_reduce_stride_lists_of_views():
    c = Sim()
    x = rng_x((2, 3, 4, 5), 2)
    v = permuted(c, x, (2, 0, 3, 1))  # shape [4, 2, 5, 3], strides [5, 60, 1, 20]
    got = ops.ReduceL2(axes=[1, 3], keep_dims=False).run(c, [v])[0]
    R.same_bits(got.numpy(), R.reduce("l2", x.transpose(2, 0, 3, 1), [1, 3], False))
    name, a = c.launches[-1]
    assert name == "rten_hip_reduce_strided" and (a[0], a[1], a[2], a[5]) == (2, 0, 1, 1)
    # kept dims 4 x 5 with strides 5, 1 merge into one of 20; reduced dims 2 x 3 with strides 60, 20 merge into one of 6 with stride 20
    assert (list(a[3])[:1], list(a[4])[:1], list(a[6])[:1], list(a[7])[:1]) == ([20], [1], [6], [20])
    got = ops.ReduceProd(axes=[0, 2], keep_dims=True).run(c, [v])[0]
    R.same_bits(got.numpy(), R.reduce("prod", x.transpose(2, 0, 3, 1), [0, 2], True))
    name, a = c.launches[-1]
    assert (a[0], a[2], a[5]) == (5, 1, 1) and (list(a[3])[:1], list(a[4])[:1], list(a[6])[:1], list(a[7])[:1]) == ([6], [20], [20], [1])
    # a step-2 slice of the last axis: stride 2, nothing merges with it
    t = dev(c, x)
    sl = E.View(t, [2, 3, 4, 3], [60, 20, 5, 2])
    got = ops.ReduceLogSumExp(axes=[3], keep_dims=False).run(c, [sl])[0]
    R.same_bits(got.numpy(), R.reduce("log_sum_exp", x[..., ::2], [3], False))
    name, a = c.launches[-1]
    assert (a[2], a[5]) == (1, 1) and (list(a[3])[:1], list(a[4])[:1], list(a[6])[:1], list(a[7])[:1]) == ([24], [5], [3], [2])


def test_lp_normalization_operator():
    c = Sim()
    x = rng_x((3, 4, 5), 5)
    x[1, :, 2] = 0
    x[2, 3, :] = 0
    for axis in (-1, 0, 1, 2, -3):
        for p in (1, 2):
            got = ops.LpNormalization(axis=axis, p=p).run(c, [dev(c, x)])[0]
            R.same_bits(got.numpy(), R.lp_normalization(x, axis, p), (axis, p))
            assert [l[0] for l in c.launches[-1:]] == ["rten_hip_lp_normalize_f32"]  # one launch per call
    op = ops.LpNormalization()
    assert (op.axis, op.p, op.max_inputs()) == (-1, 2, 1)  # onnx_registry.rs:1284-1287
    # axis 1 of [3, 4, 5]: kept dims 3 x 5 with strides 20, 1 stay apart; the lane has 4 elements 5 apart
    ops.LpNormalization(axis=1, p=1).run(c, [dev(c, x)])
    name, a = c.launches[-1]
    assert a[0] == 1 and a[1] == 2 and list(a[2])[:2] == [3, 5] and list(a[3])[:2] == [20, 1] and (a[4], a[5]) == (4, 5)
    # the last axis: the kept dims merge into one of 12 rows, 5 apart
    ops.LpNormalization().run(c, [dev(c, x)])
    name, a = c.launches[-1]
    assert a[0] == 2 and a[1] == 1 and list(a[2])[:1] == [12] and list(a[3])[:1] == [5] and (a[4], a[5]) == (5, 1)
    e = GOLDEN["errors"]["lp_normalization_p"]
    raises(lambda: ops.LpNormalization(p=e["p"]).run(c, [dev(c, x)]), ops.OpError(e["kind"], e["message"]))
    raises(lambda: ops.LpNormalization(p=3, axis=7).run(c, [dev(c, x)]), ops.UnsupportedValue("`p` must be 1 or 2"))  # p is looked at before the axis
    raises(lambda: ops.LpNormalization(axis=3).run(c, [dev(c, x)]), ops.InvalidValue("Axis is invalid"))
    raises(lambda: ops.LpNormalization().run(c, [dev(c, np.array(1.0, F))]), ops.InvalidValue("Axis is invalid"))
    raises(lambda: ops.LpNormalization().run(c, [dev(c, np.zeros(3, np.int32))]), ops.OpError("InputCastFailed", "expected float32 tensor"))
    raises(lambda: ops.LpNormalization().run(c, []), ops.MissingInputs)
    n = len(c.launches)
    assert ops.LpNormalization(axis=1).run(c, [dev(c, np.zeros((3, 0, 2), F))])[0].shape == (3, 0, 2) and len(c.launches) == n  # a zero-length axis: the input
    # a permuted view is normalised as a contiguous copy of itself
    v = permuted(c, x, (2, 0, 1))
    R.same_bits(ops.LpNormalization(axis=0).run(c, [v])[0].numpy(), R.lp_normalization(x.transpose(2, 0, 1), 0, 2))


def test_global_max_pool_operator():
    c = Sim()
    for shape in ((2, 3, 5, 7), (2, 3, 9), (2, 3), (1, 2, 2, 2, 2)):
        x = rng_x(shape, 6)
        got = ops.GlobalMaxPool().run(c, [dev(c, x)])[0]
        assert got.shape == tuple(shape[:2]) + (1,) * (len(shape) - 2)
        assert np.array_equal(select_rules.canon(got.numpy(), True), select_rules.canon(R.global_max_pool(x), True))
        name, a = c.launches[-1]
        assert name == "rten_hip_reduce_minmax_strided" and (a[0], a[1]) == (ops.SELECT_MAX, 0)  # a lowering onto the selection kernel: no new one
    x = rng_x((2, 3, 5, 7), 7)
    ops.GlobalMaxPool().run(c, [dev(c, x)])
    name, a = c.launches[-1]
    assert (a[2], a[5]) == (1, 1) and (list(a[3])[:1], list(a[4])[:1], list(a[6])[:1], list(a[7])[:1]) == ([6], [35], [35], [1])
    x[1, 2, 3, 4] = np.nan
    assert np.isnan(ops.GlobalMaxPool().run(c, [dev(c, x)])[0].numpy()[1, 2, 0, 0])
    e = GOLDEN["errors"]["global_pool_ndim"]
    raises(lambda: ops.GlobalMaxPool().run(c, [dev(c, np.zeros(4, F))]), ops.OpError(e["kind"], e["message"]))
    raises(lambda: ops.GlobalMaxPool().run(c, [dev(c, np.zeros((2, 2), np.int32))]), ops.OpError("InputCastFailed", "expected float32 tensor"))
    raises(lambda: ops.GlobalMaxPool().run(c, []), ops.MissingInputs)
    assert ops.GlobalMaxPool().max_inputs() == 1


# ------------------------------------------------------------------------------------------ 4. registries, header, bindings
NEW_OPS = ("ReduceL1", "ReduceL2", "ReduceSumSquare", "ReduceLogSum", "ReduceLogSumExp", "ReduceProd", "LpNormalization", "GlobalMaxPool")


def test_entry_points_constants_and_registries():
    so = lib.load()
    header = open(os.path.join(ROOT, "include", "rten_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rten-hip-sys", "src", "lib.rs")).read()
    for name in ("rten_hip_reduce_strided", "rten_hip_lp_normalize_f32"):
        assert hasattr(so, name) and name in lib.PROTOTYPES
        assert re.search(rf"pub fn {name}\(", rs), name
        nargs = len(re.search(rf"int32_t {name}\(([^;]*)\);", header).group(1).split(","))
        assert nargs == len(lib.PROTOTYPES[name][1]), name  # the ctypes signature has the header's arity
    for i, k in enumerate(("L1", "SUM_SQUARE", "L2", "LOG_SUM", "LOG_SUM_EXP", "PROD")):
        assert re.search(rf"^#define RTEN_HIP_REDUCE_{k} {i}\b", header, flags=re.M), k
        assert re.search(rf"pub const RTEN_HIP_REDUCE_{k}: i32 = {i};", rs), k
    assert (ops.REDUCE_L1, ops.REDUCE_SUM_SQUARE, ops.REDUCE_L2, ops.REDUCE_LOG_SUM, ops.REDUCE_LOG_SUM_EXP, ops.REDUCE_PROD) == tuple(range(6))
    assert [OPS[k].kind for k in R.KINDS] == list(range(6))
    assert re.search(r"^#define RTEN_HIP_ABI_VERSION 8\b", header, flags=re.M)  # additive: the ABI stays 8
    reg = ops.OpRegistry.with_all_ops()
    hpp = open(os.path.join(ROOT, "include", "rten_hip_ops.hpp")).read()
    for name in NEW_OPS:
        assert reg.get(name)().name() == name
        assert f'r.register_op<{name}>("{name}");' in hpp, name
