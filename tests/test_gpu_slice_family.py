"""The whole strided reduction family on ONE awkward view, through rten_amd.ops: ReduceSum / ReduceMean, the six kinds of rten_hip_reduce_strided,
ReduceMax / ReduceMin, ArgMax / ArgMin, TopK and LpNormalization all describe their slices with rten_amd/csrc/slice.h, so one view on which nothing merges
goes through every entry point, float32 and (where the operator takes it) int32.

The view: a (3, 5, 2, 7) tensor, every second element of dim 1, permuted by (3, 1, 0, 2) -> shape (7, 3, 3, 2), strides (1, 28, 70, 7).  Reducing dims 0 and 2
leaves kept dims 3 x 2 (strides 28, 7) and reduced dims 7 x 3 (strides 1, 70); reducing dim 2 alone leaves 7 x 3 x 2 (strides 1, 28, 7): no two neighbours
merge in any of them.  A second view of the same kind, (8, 3, 20, 2) with strides (1, 16, 96, 8) reduced over dim 1, has 320 slices: more than one
workgroup computes row bases in every kernel.  Results are compared bit for bit with tests/reduce_rules.py and tests/select_rules.py, and every output is
allocated inside a tests.confine.Guarded region whose other bytes must keep their fill.  The first test needs no device: the rule modules accept the views."""
import functools
import types

import numpy as np
import pytest

from tests import confine as K
from tests import reduce_rules as R
from tests import select_rules as S

F = np.float32
PERM = (3, 1, 0, 2)
# name -> (base shape, reduced axes for the operators that take several, the one axis of ArgMax / TopK / LpNormalization)
VIEWS = {"small": ((3, 5, 2, 7), [0, 2], 2), "320 slices": ((20, 6, 2, 8), [1], 1)}


def base_and_view(name, dtype):
    shape = VIEWS[name][0]
    r = np.random.default_rng(len(name)).standard_normal(shape)
    base = (r * 1e3).astype(np.int32) if dtype == np.int32 else (r * 3).astype(F)
    return base, base[:, ::2].transpose(PERM)


def view_geometry(name):
    """(shape, strides in elements) of the view on the contiguous base tensor"""
    shape = VIEWS[name][0]
    dense = K.dense(shape)
    sliced_shape, sliced_strides = (shape[0], (shape[1] + 1) // 2) + shape[2:], (dense[0], 2 * dense[1]) + dense[2:]
    return [sliced_shape[p] for p in PERM], [sliced_strides[p] for p in PERM]


def sum_rule(x, axes, mean):
    """ReduceSum / ReduceMean (reduce.rs:523-580, 1126-1165): vecmath::Sum of every slice, the reduced dims walked row-major; Mean divides by the length as f32"""
    keep = [d for d in range(x.ndim) if d not in axes]
    rows = np.ascontiguousarray(x.transpose(keep + list(axes))).reshape(int(np.prod([x.shape[d] for d in keep], dtype=np.int64)), -1)
    out = np.array([R.vec_sum(r) for r in rows], F)
    if mean:
        out = (out / F(rows.shape[1])).astype(F)
    return out.reshape([x.shape[d] for d in keep])


@functools.lru_cache(maxsize=None)
def cases(name, dtype):
    """[(label, operator factory, inputs after the view, [expected outputs])], computed once per view and element type"""
    from rten_amd import ops
    _, v = base_and_view(name, dtype)
    _, axes, ax = VIEWS[name]
    out = []
    if dtype == F:
        out.append(("ReduceSum", lambda: ops.ReduceSum(axes=axes, keep_dims=False), [], [sum_rule(v, axes, False)]))
        out.append(("ReduceMean", lambda: ops.ReduceMean(axes=axes, keep_dims=False), [], [sum_rule(v, axes, True)]))
        for p in (1, 2):
            out.append((f"LpNormalization p={p}", lambda p=p: ops.LpNormalization(axis=ax, p=p), [], [R.lp_normalization(v, ax, p)]))
    from tests.test_reduce_ops import OPS
    for kind in (R.KINDS if dtype == F else R.INT32_KINDS):
        xk = (np.abs(v) + F(0.25)).astype(F) if kind == "log_sum" else v
        out.append((f"Reduce {kind}", lambda kind=kind: OPS[kind](axes=axes, keep_dims=False), [], [R.reduce(kind, xk, axes, False)], kind == "log_sum"))
    for op, cls in (("max", ops.ReduceMax), ("min", ops.ReduceMin)):
        out.append((f"Reduce{op}", lambda cls=cls: cls(axes=axes, keep_dims=False), [], [S.reduce_minmax(v, axes, False, op)]))
    for op, cls in (("max", ops.ArgMax), ("min", ops.ArgMin)):
        out.append((f"Arg{op}", lambda cls=cls: cls(axis=ax, keep_dims=False), [], [S.arg_minmax(v, ax, False, op)]))
    for largest in (True, False):
        out.append((f"TopK largest={largest}", lambda largest=largest: ops.TopK(axis=ax, largest=largest), [np.array([2], np.int32)], list(S.topk(v, 2, ax, largest))))
    return out


@pytest.mark.parametrize("name", list(VIEWS))
def test_the_views_do_not_merge_and_the_rules_take_them(name):
    from rten_amd import ops
    shape, strides = view_geometry(name)
    base, v = base_and_view(name, F)
    assert list(v.shape) == shape and [s // 4 for s in v.strides] == strides
    fake = types.SimpleNamespace(shape=shape, strides=strides)
    _, axes, ax = VIEWS[name]
    keep, osh, (ost,), ish, ist = ops._split_dims(fake, axes)
    assert osh == [shape[d] for d in keep] and ish == [shape[d] for d in axes] and ost == [strides[d] for d in keep] and ist == [strides[d] for d in axes]
    keep, osh, (ost,), ish, ist = ops._split_dims(fake, [ax])
    assert osh == [shape[d] for d in keep] and len(osh) == 3 and ost == [strides[d] for d in keep]
    if name == "small":
        assert (shape, strides, osh, ost) == ([7, 3, 3, 2], [1, 28, 70, 7], [7, 3, 2], [1, 28, 7])
    else:
        assert int(np.prod(osh)) == 320 > 256
    for dtype in (F, np.int32):
        for case in cases(name, dtype):
            assert all(w.size for w in case[3]), case[0]
    assert v.size <= 1000


class GuardedOutputs:
    """While installed, every tensor rten_amd.ops and rten_amd.einsum allocate sits in a tests.confine.Guarded region of its own."""

    def __init__(self, monkeypatch):
        from rten_amd import einsum, ops
        from rten_amd.tensor import DeviceTensor
        self.regions = []

        def alloc(ctx, shape, dtype=np.float32, ptr=None, keepalive=None):
            if ptr is not None:
                return DeviceTensor(ctx, shape, dtype, ptr=ptr, keepalive=keepalive)
            dtype = np.dtype(dtype)
            g = K.Guarded(ctx, int(np.prod(shape, dtype=np.int64)) * dtype.itemsize, itemsize=dtype.itemsize)
            self.regions.append(g)
            return g.tensor(shape, dtype)

        alloc.from_numpy = DeviceTensor.from_numpy
        monkeypatch.setattr(ops, "DeviceTensor", alloc)
        monkeypatch.setattr(einsum, "DeviceTensor", alloc)

    def contents(self, t, what):
        """The output tensor `t` read back from its region, after the check that nothing else of the region changed"""
        (g,) = [g for g in self.regions if g.ptr == t.ptr]
        return g.check(g.raw(), t.shape, K.dense(t.shape), t.dtype, what)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.int32])
@pytest.mark.parametrize("name", list(VIEWS))
def test_every_entry_point_on_the_view(ctx, monkeypatch, name, dtype):
    from rten_amd import einsum as E
    from rten_amd.tensor import DeviceTensor
    base, v = base_and_view(name, dtype)
    shape, strides = view_geometry(name)
    guard = GuardedOutputs(monkeypatch)
    for case in cases(name, dtype):
        label, make, extra, want = case[:4]
        src = (np.abs(base) + F(0.25)).astype(F) if len(case) > 4 and case[4] else base  # ReduceLogSum: positive sums
        t = DeviceTensor.from_numpy(ctx, np.ascontiguousarray(src))
        got = make().run(ctx, [E.View(t, shape, strides)] + extra)
        ctx.sync()
        assert len(got) == len(want), label
        for g, w in zip(got, want):
            what = f"{label} on the {name} view, {np.dtype(dtype).name}"
            R.same_bits(guard.contents(g, what), w, what)
