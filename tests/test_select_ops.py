"""ReduceMax / ReduceMin / ArgMax / ArgMin / TopK without a GPU: (1) the numpy restatement of the rules (tests/select_rules.py) against the literals of the
reference's own tests (src/ops/reduce.rs:1386-1496, 2009-2051, 2245-2388); (2) the Python operators' host logic -- shapes, keepdims, axes resolution, the
stride lists handed to the C ABI, every error -- on a simulated context whose three entry points ARE the restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rten_amd import einsum as E
from rten_amd import lib, ops
from rten_amd.tensor import DeviceTensor
from tests import select_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
F = np.float32


def f32(v):
    return np.array(v, F)


def same(got, want, fold_zero_sign=False):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert np.array_equal(R.canon(got, fold_zero_sign), R.canon(want, fold_zero_sign)), (got, want)


# ------------------------------------------------------------------------------------------ 1. restatement vs the reference's literals
PROBS = [0.1, 0.5, 0.2, 0.9, 0.01, 0.6]
ITEMS = [[[0.1, 0.2, 0.9], [0.9, 0.1, 0.2], [0.3, 0.8, 0.4], [0.1, 0.01, 0.2]]]


def test_arg_max_literals():  # test_arg_max, reduce.rs:1386-1466
    same(R.arg_minmax(f32(PROBS), 0, False), np.array(3, np.int32))
    same(R.arg_minmax(f32(PROBS), 0, True), np.array([3], np.int32))
    same(R.arg_minmax(f32(ITEMS), 2, False), np.array([[2, 0, 1, 2]], np.int32))
    same(R.arg_minmax(f32(ITEMS), 2, True), np.array([[[2], [0], [1], [2]]], np.int32))
    same(R.arg_minmax(np.zeros((10, 0, 5), F), 0, False), np.zeros((0, 5), np.int32))
    with pytest.raises(R.RuleError, match="^Cannot select index from empty sequence$"):
        R.arg_minmax(np.zeros((10, 0, 5), F), 1, False)
    same(R.arg_minmax(f32([[1, 2], [4, 8], [5, 6]]), 0, False), np.array([2, 1], np.int32))


def test_arg_min_and_nan_literals():  # test_arg_min, test_arg_min_max_nan, reduce.rs:1470-1496
    same(R.arg_minmax(f32(PROBS), 0, False, "min"), np.array(4, np.int32))
    nan = f32([0.1, 0.5, NAN, 0.9, 0.01, 0.6])
    same(R.arg_minmax(nan, 0, False, "min"), np.array(2, np.int32))
    same(R.arg_minmax(nan, 0, False, "max"), np.array(2, np.int32))


def test_arg_tie_rules():  # Iterator::max_by keeps the later of equal elements; cmp_nan_greater keeps the first NaN
    assert R.arg_minmax(f32([1, 3, 3]), 0, False) == 2
    assert R.arg_minmax(f32([2, 1, 1]), 0, False, "min") == 2
    assert R.arg_minmax(f32([NAN, 5, NAN]), 0, False) == 0
    assert R.arg_minmax(f32([NAN, 5, NAN]), 0, False, "min") == 0
    assert R.arg_minmax(f32([-0.0, 0.0]), 0, False) == 1
    assert R.arg_minmax(f32([0.0, -0.0]), 0, False) == 1
    assert R.arg_minmax(np.array([7, 7, -3, 7], np.int32), 0, False) == 3


def test_reduce_min_max_literals():  # test_reduce_min_max, test_reduce_min_max_propagates_nan, reduce.rs:2009-2051
    x = f32([1.5, 2.5, 3.5, 4.5, 5.5])
    same(R.reduce_minmax(x, [0], False, "min"), f32(1.5))
    same(R.reduce_minmax(x, [0], False, "max"), f32(5.5))
    xn = f32([1.5, 2.5, 3.5, NAN, 5.5])
    assert np.isnan(R.reduce_minmax(xn, [0], False, "min")) and np.isnan(R.reduce_minmax(xn, [0], False, "max"))
    # identities of an empty reduction, and a 0-d input
    same(R.reduce_minmax(np.zeros((2, 0), F), [1], False, "max"), f32([-np.inf, -np.inf]))
    same(R.reduce_minmax(np.zeros((2, 0), np.int32), [1], True, "min"), np.full((2, 1), 2**31 - 1, np.int32))
    same(R.reduce_minmax(f32(4.0), None, True, "max"), f32(4.0))


TOPK_CASES = [  # (input, k, axis, largest, values, indices): test_topk, reduce.rs:2245-2388
    ([0., 1., 2.], 2, None, True, [2., 1.], [2, 1]),
    ([0., 1., 2.], 2, None, False, [0., 1.], [0, 1]),
    ([0., 1., 2.], 0, None, True, [], []),
    ([1., 0., 2., 3., 1.], 5, None, True, [3., 2., 1., 1., 0.], [3, 2, 0, 4, 1]),
    ([1., 0., 2., 3., 1.], 5, None, False, [0., 1., 1., 2., 3.], [1, 0, 4, 2, 3]),
    ([0., NAN, 2.], 2, None, True, [NAN, 2.], [1, 2]),
    ([0., NAN, 2.], 3, None, False, [0., 2., NAN], [0, 2, 1]),
    ([[0., 1., 2.], [0., 1., 3.], [0., 1., 4.]], 2, None, True, [[2., 1.], [3., 1.], [4., 1.]], [[2, 1], [2, 1], [2, 1]]),
    ([[0., 1., 2.], [3., 4., 5.], [6., 7., 8.]], 2, 0, True, [[6., 7., 8.], [3., 4., 5.]], [[2, 2, 2], [1, 1, 1]]),
]


@pytest.mark.parametrize("case", range(len(TOPK_CASES)))
def test_topk_literals(case):
    x, k, axis, largest, values, indices = TOPK_CASES[case]
    v, i = R.topk(f32(x), k, axis, largest)
    same(v, f32(values))
    same(i, np.array(indices, np.int32))


def test_topk_error_literals():
    with pytest.raises(R.RuleError, match="^k > dimension size$"):
        R.topk(f32([0., 1., 2.]), 4)
    with pytest.raises(R.RuleError, match="^Axis is invalid$"):
        R.topk(f32(0.), 2)
    with pytest.raises(R.RuleError, match="^k must be positive$"):
        R.topk(f32([0., 1.]), -1)


# ------------------------------------------------------------------------------------------ 2. host logic on a simulated context
class SimCtx:
    """Context.call on host memory: the allocator, the strided copy and the three selection entry points (= the restatement).  Launches are recorded."""

    def __init__(self):
        self.heap, self.launches, self.h = {}, [], 1

    @staticmethod
    def _addr(p):
        return p if isinstance(p, int) else (p.value or 0) if p is not None else 0

    @staticmethod
    def _view(addr, shape, strides, dtype):
        shape, strides = [int(s) for s in shape], [int(s) for s in strides]
        if any(s == 0 for s in shape):
            return np.zeros(shape, dtype)
        n = 1 + sum((s - 1) * st for s, st in zip(shape, strides))
        flat = np.ctypeslib.as_array((C.c_uint32 * n).from_address(addr)).view(dtype)
        return np.lib.stride_tricks.as_strided(flat, shape=shape, strides=[4 * s for s in strides])

    def call(self, name, *a):
        val = lambda v: int(v.value if hasattr(v, "value") else v)
        if name == "rten_hip_malloc":
            buf = np.full(val(a[0]) + 64, 0xCD, np.uint8)
            self.heap[buf.ctypes.data] = buf
            a[1]._obj.value = buf.ctypes.data
            return
        if name == "rten_hip_free":
            self.heap.pop(self._addr(a[0]), None)
            return
        if name in ("rten_hip_memcpy_h2d", "rten_hip_memcpy_d2h"):
            C.memmove(self._addr(a[0]), self._addr(a[1]), val(a[2]))
            return
        self.launches.append((name, a))
        dts = {0: np.float32, 1: np.int32}
        if name == "rten_hip_copy_strided_b32":
            nd, shape, st, x, y = a
            shape = list(shape)[:nd]
            self._view(self._addr(y), shape, _row_major(shape), np.uint32)[...] = self._view(self._addr(x), shape, list(st)[:nd], np.uint32)
        elif name == "rten_hip_reduce_minmax_strided":
            op, dt, no, osh, ost, ni, ish, ist, x, y = a
            assert no <= 6 and ni <= 6
            osh, ost, ish, ist = list(osh)[:no], list(ost)[:no], list(ish)[:ni], list(ist)[:ni]
            v = self._view(self._addr(x), osh + ish, ost + ist, dts[dt])
            out = self._view(self._addr(y), osh, _row_major(osh), dts[dt])
            out[...] = R.reduce_minmax(v, list(range(no, no + ni)), False, ("max", "min")[op]) if ni else v
        elif name == "rten_hip_arg_minmax_strided":
            op, dt, no, osh, ost, n, st, x, y = a
            osh, ost = list(osh)[:no], list(ost)[:no]
            v = self._view(self._addr(x), osh + [n], ost + [st], dts[dt])
            self._view(self._addr(y), osh, _row_major(osh), np.int32)[...] = R.arg_minmax(v, no, False, ("max", "min")[op])
        elif name == "rten_hip_topk_strided":
            largest, dt, no, osh, ost, oost, n, st, k, x, vals, idx, ast = a
            osh, ost, oost = list(osh)[:no], list(ost)[:no], list(oost)[:no]
            v = self._view(self._addr(x), osh + [n], ost + [st], dts[dt])
            tv, ti = R.topk(v, k, -1, bool(largest))
            self._view(self._addr(vals), osh + [k], oost + [ast], dts[dt])[...] = tv
            self._view(self._addr(idx), osh + [k], oost + [ast], np.int32)[...] = ti
        else:
            raise AssertionError(f"unexpected device call {name}")


def _row_major(shape):
    st, acc = [0] * len(shape), 1
    for i in range(len(shape) - 1, -1, -1):
        st[i] = acc
        acc *= shape[i]
    return st


def dev(ctx, a):
    return DeviceTensor.from_numpy(ctx, a)


def permuted(ctx, a, perm):
    """The view of `a` (uploaded as it is) with axes permuted: what a Transpose that was never materialised looks like."""
    t = dev(ctx, a)
    base = _row_major(a.shape)
    return E.View(t, [a.shape[p] for p in perm], [base[p] for p in perm])


def raises(fn, err):
    with pytest.raises(ops.OpError) as e:
        fn()
    assert e.value == err, (e.value, err)


def rng_f32(shape, seed=0):
    return np.random.default_rng(seed).integers(-4, 5, size=shape).astype(F)  # heavy ties on purpose


def test_entry_points_constants_and_registry():
    so = lib.load()
    header = open(os.path.join(ROOT, "include", "rten_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rten-hip-sys", "src", "lib.rs")).read()
    for name in ("rten_hip_reduce_minmax_strided", "rten_hip_arg_minmax_strided", "rten_hip_topk_strided"):
        assert hasattr(so, name) and name in lib.PROTOTYPES
        assert re.search(rf"pub fn {name}\(", rs), name
    assert re.search(r"^#define RTEN_HIP_SELECT_MAX 0\b", header, flags=re.M) and re.search(r"^#define RTEN_HIP_SELECT_MIN 1\b", header, flags=re.M)
    assert (ops.SELECT_MAX, ops.SELECT_MIN) == (0, 1)
    assert re.search(r"^#define RTEN_HIP_ABI_VERSION 8\b", header, flags=re.M)
    reg = ops.OpRegistry.with_all_ops()
    for name in ("ReduceMax", "ReduceMin", "ArgMax", "ArgMin", "TopK"):
        assert reg.get(name)().name() == name
    a, t, r = ops.ArgMax(), ops.TopK(), ops.ReduceMax()
    assert (a.axis, a.keep_dims) == (0, True) and (t.axis, t.largest, t.sorted) == (-1, True, True)
    assert (r.axes, r.keep_dims, r.noop_with_empty_axes) == (None, True, False)
    raises(lambda: ops.ArgMax(select_last_index=1), ops.UnsupportedValue("select_last_index is not supported"))
    raises(lambda: ops.ArgMin(select_last_index=1), ops.UnsupportedValue("select_last_index is not supported"))


@pytest.mark.parametrize("dtype", [np.float32, np.int32])
def test_reduce_shapes_axes_keepdims(dtype):
    c = SimCtx()
    x = rng_f32((2, 3, 4, 5)).astype(dtype)
    for cls, op in ((ops.ReduceMax, "max"), (ops.ReduceMin, "min")):
        for axes in (None, [], [0], [3], [-1], [1, 2], [2, 1, -2], [0, 1, 2, 3], [-4, 3]):
            for keep in (True, False):
                got = cls(axes=axes, keep_dims=keep).run(c, [dev(c, x)])[0]
                same(got.numpy(), R.reduce_minmax(x, axes, keep, op))
                # axes as the second input override the attribute
                got = cls(axes=[0], keep_dims=keep).run(c, [dev(c, x), None if axes is None else np.array(axes, np.int32)])[0]
                same(got.numpy(), R.reduce_minmax(x, [0] if axes is None else axes, keep, op))
        same(cls(axes=[], noop_with_empty_axes=True).run(c, [dev(c, x)])[0].numpy(), x)
        same(cls(noop_with_empty_axes=True).run(c, [dev(c, x)])[0].numpy(), x)
        same(cls().run(c, [dev(c, np.array(3, dtype))])[0].numpy(), np.array(3, dtype))  # 0-d returns itself
        raises(lambda: cls(axes=[4]).run(c, [dev(c, x)]), ops.InvalidValue("Axis is invalid"))
        raises(lambda: cls(axes=[-5]).run(c, [dev(c, x)]), ops.InvalidValue("Axis is invalid"))
        raises(lambda: cls().run(c, []), ops.MissingInputs)
        # empty slices give the identity; an empty output launches nothing
        e = np.zeros((2, 0, 3), dtype)
        same(cls(axes=[1], keep_dims=False).run(c, [dev(c, e)])[0].numpy(), R.reduce_minmax(e, [1], False, op))
        n = len(c.launches)
        assert cls(axes=[0]).run(c, [dev(c, e)])[0].shape == (1, 0, 3) and len(c.launches) == n
    raises(lambda: ops.ReduceMax().run(c, [dev(c, np.zeros(3, np.uint8))]), ops.UnsupportedType)


def test_reduce_stride_lists_of_a_permuted_view():
    c = SimCtx()
    x = rng_f32((2, 3, 4, 5), 1)
    v = permuted(c, x, (2, 0, 3, 1))  # shape [4, 2, 5, 3], strides [5, 60, 1, 20]
    got = ops.ReduceMax(axes=[1, 3], keep_dims=False).run(c, [v])[0]
    same(got.numpy(), R.reduce_minmax(x.transpose(2, 0, 3, 1), [1, 3], False))
    name, a = c.launches[-1]
    assert name == "rten_hip_reduce_minmax_strided" and (a[0], a[1], a[2], a[5]) == (0, 0, 1, 1)
    # kept dims 4 x 5 with strides 5, 1 merge into one of 20; reduced dims 2 x 3 with strides 60, 20 merge into one of 6 with stride 20
    assert (list(a[3])[:1], list(a[4])[:1], list(a[6])[:1], list(a[7])[:1]) == ([20], [1], [6], [20])
    got = ops.ReduceMin(axes=[0, 2], keep_dims=True).run(c, [v])[0]
    same(got.numpy(), R.reduce_minmax(x.transpose(2, 0, 3, 1), [0, 2], True, "min"))
    name, a = c.launches[-1]
    assert (a[0], a[2], a[5]) == (1, 1, 1) and (list(a[3])[:1], list(a[4])[:1], list(a[6])[:1], list(a[7])[:1]) == ([6], [20], [20], [1])  # the mirror image
    # axes that do not merge stay apart: reducing dim 2 of the view keeps 4 x 2 x 3 with strides 5, 60, 20
    ops.ReduceMax(axes=[2], keep_dims=False).run(c, [v])
    name, a = c.launches[-1]
    assert a[2] == 2 and list(a[3])[:2] == [4, 6] and list(a[4])[:2] == [5, 20] and (list(a[6])[:1], list(a[7])[:1]) == ([5], [1])
    # TopK walks the kept dims through two stride lists, the view's and its contiguous outputs' (the table tests/cpp/test_reduce_hostops.cpp holds for C++):
    # along dim 2 of the view, k = 2, the outputs are [4, 2, 2, 3] with strides 12, 6, 3, 1 -- kept 2 x 3 would merge in the view (60 = 20 * 3), not in them
    K = np.array([2], np.int32)
    tv, ti = ops.TopK(axis=2).run(c, [v, K])
    wv, wi = R.topk(x.transpose(2, 0, 3, 1), 2, 2)
    same(tv.numpy(), wv)
    same(ti.numpy(), wi)
    name, a = c.launches[-1]
    assert name == "rten_hip_topk_strided" and a[2] == 3 and (list(a[3])[:3], list(a[4])[:3], list(a[5])[:3]) == ([4, 2, 3], [5, 60, 20], [12, 6, 1])
    assert (a[6], a[7], a[8], a[12]) == (5, 1, 2, 3)
    # along the last dim of the contiguous tensor every kept dim merges in both lists: 24 lanes, 5 apart in the input and 2 apart in the outputs
    ops.TopK(axis=3).run(c, [dev(c, x), K])
    name, a = c.launches[-1]
    assert a[2] == 1 and (list(a[3])[:1], list(a[4])[:1], list(a[5])[:1]) == ([24], [5], [2]) and (a[6], a[7], a[8], a[12]) == (5, 1, 2, 1)


@pytest.mark.parametrize("dtype", [np.float32, np.int32])
def test_arg_shapes_and_errors(dtype):
    c = SimCtx()
    x = rng_f32((3, 4, 5), 2).astype(dtype)
    for cls, op in ((ops.ArgMax, "max"), (ops.ArgMin, "min")):
        for axis in (0, 1, 2, -1, -3):
            for keep in (True, False):
                got = cls(axis=axis, keep_dims=keep).run(c, [dev(c, x)])[0]
                same(got.numpy(), R.arg_minmax(x, axis, keep, op))
        same(cls().run(c, [dev(c, x)])[0].numpy(), R.arg_minmax(x, 0, True, op))  # defaults: axis 0, keepdims
        raises(lambda: cls(axis=3).run(c, [dev(c, x)]), ops.InvalidValue("Axis is invalid"))
        raises(lambda: cls(axis=0).run(c, [dev(c, np.array(1, dtype))]), ops.InvalidValue("Axis is invalid"))
        e = np.zeros((10, 0, 5), dtype)
        raises(lambda: cls(axis=1).run(c, [dev(c, e)]), ops.InvalidValue("Cannot select index from empty sequence"))
        got = cls(axis=0, keep_dims=False).run(c, [dev(c, e)])[0]
        assert got.shape == (0, 5) and got.dtype == np.int32
        raises(lambda: cls().run(c, []), ops.MissingInputs)
    v = permuted(c, x, (2, 0, 1))  # shape [5, 3, 4], strides [1, 20, 5]
    same(ops.ArgMax(axis=1, keep_dims=False).run(c, [v])[0].numpy(), R.arg_minmax(x.transpose(2, 0, 1), 1, False))
    name, a = c.launches[-1]
    assert name == "rten_hip_arg_minmax_strided" and a[2] == 2 and list(a[3])[:2] == [5, 4] and list(a[4])[:2] == [1, 5] and (a[5], a[6]) == (3, 20)
    nan = f32([[NAN, 5, NAN], [1, 3, 3], [-0.0, 0.0, -1]])
    same(ops.ArgMax(axis=1, keep_dims=False).run(c, [dev(c, nan)])[0].numpy(), np.array([0, 2, 1], np.int32))


@pytest.mark.parametrize("dtype", [np.float32, np.int32])
def test_topk_shapes_and_errors(dtype):
    c = SimCtx()
    x = rng_f32((3, 6, 4), 3).astype(dtype)
    K = lambda k: np.array([k], np.int32)
    for axis in (None, -1, 0, 1, 2):
        for largest in (True, False):
            for k in (1, 3):
                v, i = ops.TopK(axis=axis, largest=largest).run(c, [dev(c, x), K(k)])
                wv, wi = R.topk(x, k, axis, largest)
                same(v.numpy(), wv)
                same(i.numpy(), wi)
    v, i = ops.TopK().run(c, [dev(c, x), np.array(0, np.int32)])  # k == 0: two empty tensors, no launch
    assert v.shape == i.shape == (3, 6, 0) and v.dtype == dtype and i.dtype == np.int32
    raises(lambda: ops.TopK().run(c, [dev(c, x), K(5)]), ops.InvalidValue("k > dimension size"))
    raises(lambda: ops.TopK().run(c, [dev(c, x), K(-1)]), ops.InvalidValue("k must be positive"))
    raises(lambda: ops.TopK().run(c, [dev(c, np.array(0, dtype)), K(2)]), ops.InvalidValue("Axis is invalid"))
    raises(lambda: ops.TopK(axis=3).run(c, [dev(c, x), K(1)]), ops.InvalidValue("Axis is invalid"))
    raises(lambda: ops.TopK().run(c, [dev(c, x)]), ops.MissingInputs)
    # axis 0 of a matrix: lanes strided by the row length, the outputs' lanes by theirs
    m = rng_f32((5, 7), 4).astype(dtype)
    v, i = ops.TopK(axis=0).run(c, [dev(c, m), K(2)])
    same(v.numpy(), R.topk(m, 2, 0)[0])
    name, a = c.launches[-1]
    assert name == "rten_hip_topk_strided" and a[2] == 1 and (list(a[3])[:1], list(a[4])[:1], list(a[5])[:1]) == ([7], [1], [1]) and (a[6], a[7], a[8], a[12]) == (5, 7, 2, 7)


def test_topk_reference_cases_through_the_operator():
    c = SimCtx()
    for x, k, axis, largest, values, indices in TOPK_CASES:
        v, i = ops.TopK(axis=axis, largest=largest).run(c, [dev(c, f32(x)), np.array(k, np.int32)])
        same(v.numpy(), f32(values))
        same(i.numpy(), np.array(indices, np.int32))
