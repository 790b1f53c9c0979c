"""The glue operators without a GPU: the rules (tests/glue_rules.py) against the literals of the reference's own unit tests
(tests/golden/glue_reference.json), the table of cases (tests/glue_cases.py) against what it must contain, and the host path -- hostops::* of
include/rten_hip_graph.hpp, through the g++ program tests/cpp/test_glue_hostops.cpp -- against the rules over the whole table, bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import glue_cases as T
from tests import glue_rules as R
from tests.math_rules import RuleError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "glue_reference.json")))
F, I32 = np.float32, np.int32
_SPECIAL = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "-0.0": -0.0}


def _arr(v, shape=None, dtype=np.float32):
    a = np.array([_SPECIAL.get(e, e) if isinstance(e, str) else e for e in v], dtype)
    return a.reshape(shape) if shape is not None else a


def _check(case, run, dtype=None, exact=True):
    """`run()` reproduces the case's expected shape / values, or raises its error."""
    if "error" in case:
        with pytest.raises(RuleError) as e:
            run()
        assert [e.value.kind, e.value.msg] == case["error"]
        return
    y = run()
    if "expected_shape" in case:
        assert list(y.shape) == case["expected_shape"], y.shape
    if dtype is not None:
        assert y.dtype == np.dtype(dtype)
    if "expected" in case:
        want = _arr(case["expected"], None, y.dtype)
        if exact:
            assert np.array_equal(y.ravel(), want, equal_nan=True), (y, want)
        else:  # rten_tensor::test_util::expect_equal: |a - b| <= 1e-4
            assert np.abs(y.ravel() - want).max() <= 1e-4


_ids = lambda c: c["cite"].split(" ", 1)[1][:60].replace(" ", "-")


# ---------------------------------------------------------------------------------------------- 1. the rules against the reference's literals
@pytest.mark.parametrize("case", GOLDEN["slice"], ids=_ids)
def test_slice_rules_reproduce_the_reference_literals(case):
    x = _arr(case["input"], case["shape"], case["dtype"])
    _check(case, lambda: R.slice(x, case["starts"], case["ends"], case.get("axes"), case.get("steps")), case["dtype"])


@pytest.mark.parametrize("case", GOLDEN["gather"], ids=_ids)
def test_gather_rules_reproduce_the_reference_literals(case):
    x = _arr(case["input"], case["shape"], case["dtype"])
    ids = _arr(case["indices"], case["indices_shape"], I32)
    _check(case, lambda: R.gather(x, ids, case["axis"]), case["dtype"])


@pytest.mark.parametrize("case", GOLDEN["range"], ids=_ids)
def test_range_rules_reproduce_the_reference_literals(case):
    t = np.dtype(case["dtype"]).type
    _check(case, lambda: R.range_(t(case["start"]), t(case["limit"]), t(case["delta"])), case["dtype"])


@pytest.mark.parametrize("case", GOLDEN["constant_of_shape"], ids=_ids)
def test_constant_of_shape_rules_reproduce_the_reference_literals(case):
    value = np.dtype(case["value_dtype"]).type(case["value"])
    _check(case, lambda: R.constant_of_shape(case["shape"], value), case["value_dtype"])
    if "expected_fill" in case:
        assert (R.constant_of_shape(case["shape"], value) == case["expected_fill"]).all()


@pytest.mark.parametrize("case", GOLDEN["expand"], ids=_ids)
def test_expand_rules_reproduce_the_reference_literals(case):
    _check(case, lambda: R.expand(_arr(case["input"], case["shape"], I32), case["target"]), I32)


@pytest.mark.parametrize("case", GOLDEN["concat"], ids=_ids)
def test_concat_rules_reproduce_the_reference_literals(case):
    xs = [_arr(v, s, case["dtype"]) for v, s in zip(case["inputs"], case["shapes"])]
    _check(case, lambda: R.concat(xs, case["axis"]), case["dtype"])


@pytest.mark.parametrize("case", GOLDEN["cast"], ids=_ids)
def test_cast_rules_reproduce_the_reference_literals(case):
    _check(case, lambda: R.cast(_arr(case["input"], None, case["from"]), case["to"]), case["to"])


@pytest.mark.parametrize("case", GOLDEN["div"], ids=_ids)
def test_div_rules_reproduce_the_reference_literals(case):
    a, b = _arr(case["a"], case["a_shape"], case["dtype"]), _arr(case["b"], case["b_shape"], case["dtype"])
    _check(case, lambda: (R.div_f32 if case["dtype"] == "float32" else R.idiv)(a, b), case["dtype"], exact=not case.get("approx"))


@pytest.mark.parametrize("case", GOLDEN["nonzero"], ids=_ids)
def test_nonzero_rules_reproduce_the_reference_literals(case):
    _check(case, lambda: R.nonzero(_arr(case["input"], case["shape"], case["dtype"])), I32)


@pytest.mark.parametrize("case", GOLDEN["reshape"], ids=_ids)
def test_reshape_rules_reproduce_the_reference_literals(case):
    _check(case, lambda: R.reshape(np.zeros(case["input_shape"], F), case["shape"], case["allow_zero"]), F)


@pytest.mark.parametrize("case", GOLDEN["views"], ids=_ids)
def test_view_rules_reproduce_the_reference_literals(case):
    x = np.zeros(case["input_shape"], F)
    run = {"squeeze": lambda: R.squeeze(x, case["axes"]), "unsqueeze": lambda: R.unsqueeze(x, case["axes"]), "transpose": lambda: R.transpose(x, case["perm"])}[case["op"]]
    _check(case, run, F)


# ---------------------------------------------------------------------------------------------- 2. the rules against independent statements
def test_slice_rule_is_python_slicing_wherever_python_defines_it():
    x = np.arange(7, dtype=I32)
    edges = [None, 0, 1, 3, 6, 7, 8, 100, -1, -2, -6, -7, -8, -100]
    big = lambda v, step, is_start: v if v is not None else ((-(1 << 40) if step > 0 else (1 << 40)) if is_start else ((1 << 40) if step > 0 else -(1 << 40)))
    for step in (1, 2, 3, -1, -2, -3):
        for s in edges:
            for e in edges:
                got = R.slice(x, [big(s, step, True)], [big(e, step, False)], [0], [step])
                assert np.array_equal(got, x[s:e:step]), (s, e, step, got)


def test_one_element_divisor_rule_differs_from_a_division_where_the_issue_says():
    x = np.random.default_rng(3).standard_normal(100000).astype(F)
    frac = lambda d: float(np.mean(R.div_f32(x, F(d)).view(I32) != (x / F(d)).view(I32)))
    assert 0.30 < frac(3) < 0.37 and 0.37 < frac(1.4142135) < 0.45 and 0.10 < frac(0.1) < 0.18 and frac(8) == 0.0
    two = np.array([3.0, 3.0], F)
    assert R.same_bits(R.div_f32(x.reshape(-1, 2), two), x.reshape(-1, 2) / two)          # two elements: a division
    assert R.same_bits(R.div_f32(F(3), x), (F(3) / x).astype(F))                          # the rule reads the RIGHT operand only
    for shape in ((), (1,), (1, 1, 1)):
        assert R.same_bits(R.div_f32(x, np.full(shape, 3, F)).ravel(), x * (F(1) / F(3)))


def test_float_range_accumulates():
    r = R.range_(F(0), F(1), F(0.1))
    linear = (F(0) + np.arange(10, dtype=F) * F(0.1)).astype(F)
    assert r.size == 10 and np.flatnonzero(r.view(I32) != linear.view(I32)).tolist() == [7, 8, 9]   # the last bit of elements 7 to 9
    assert R.range_(F(0), F(0.7), F(0.1)).size == 7


def test_cast_rules_are_rust_as():
    f = np.array([2147483520.0, 2147483648.0, -2147483648.0, 3e10, -3e10, np.nan, 0.9, -0.9], F)
    assert R.cast(f, I32).tolist() == [2147483520, 2147483647, -2147483648, 2147483647, -2147483648, 0, 0, 0]
    assert R.cast(np.array([255.0, 255.5, 256.0, -0.9, np.nan], F), np.uint8).tolist() == [255, 255, 255, 0, 0]
    assert R.cast(np.array([127.9, -128.9, -129.0], F), np.int8).tolist() == [127, -128, -128]
    assert R.cast(np.array([(1 << 24) + 1, 2147483647, -2147483648], I32), F).tolist() == [16777216.0, 2147483648.0, -2147483648.0]
    assert R.cast(np.arange(256, dtype=np.uint8), np.int8).tolist() == list(range(128)) + list(range(-128, 0))
    assert R.cast(np.array([256, -1, -129], I32), np.uint8).tolist() == [0, 255, 127]


# ---------------------------------------------------------------------------------------------- 3. what the table must contain
def test_table_holds_the_cases_every_evaluator_needs():
    cases = T.table()
    ids = {c.id for c in cases}
    assert len(ids) == len(cases)
    ops = {c.op for c in cases}
    assert ops >= T.HOST_PROGRAM_OPS | {"Squeeze", "Unsqueeze", "Reshape", "Flatten"}
    ranks = {a.ndim for c in cases for a in c.inputs if a is not None}
    assert {0, 1, 6, 7} <= ranks
    extents = {a.size for c in cases for a in c.inputs if a is not None}
    assert {1, 255, 256, 257, T.PAST_CAP, T.HOST_CONST, T.HOST_CONST + 1} <= extents
    assert any(a is not None and a.shape == (3, 0, 4) for c in cases for a in c.inputs)
    for c in cases:  # a rank-7 case is a refusal, never values
        if any(a is not None and a.ndim == 7 for a in c.inputs):
            assert c.want_host is None and isinstance(c.want_dev, tuple) and c.want_dev[0] == "error", c.id
    pairs = {}
    for c in cases:
        if c.pair:
            pairs.setdefault(c.pair, []).append(c)
    assert len(pairs) >= 14 and all(len(v) == 2 and v[0].hosted and not v[1].hosted for v in pairs.values())
    assert all(cid in ids for cid in T.FUSION_SUBSET)
    assert {T.by_id(cid).op for cid in T.FUSION_SUBSET} >= ops - {"Or", "LessOrEqual", "Greater", "GreaterOrEqual"}


# ---------------------------------------------------------------------------------------------- 4. the host path (a g++ program) against the rules
GLUE_BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_glue_hostops")


def build_glue_hostops_binary():
    from rten_amd import lib as L
    L.load()
    os.makedirs(os.path.dirname(GLUE_BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_glue_hostops.cpp")
    deps = [src] + [os.path.join(ROOT, "include", h) for h in ("rten_hip_graph.hpp", "rten_hip_ops.hpp", "rten_hip.h")]
    if not os.path.exists(GLUE_BIN) or os.path.getmtime(GLUE_BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", GLUE_BIN, "-L" + os.path.join(ROOT, "rten_amd"),
                               "-lrten_hip", "-Wl,-rpath,$ORIGIN/../../../rten_amd", "-Wl,-rpath," + os.path.join(ROOT, "rten_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return GLUE_BIN


def _words(a):
    """An operand as the loader hands it to the host path: float32 words, or integers narrowed to int32 (int64 saturates)."""
    a = a if a.dtype == F else R.sat32(a)
    return ("f" if a.dtype == F else "i"), np.ascontiguousarray(a).view(np.uint32).ravel()


def write_host_cases(path, cases):
    with open(path, "w") as f:
        for c in cases:
            f.write(f"CASE {c.id} {c.op}\n")
            for k, v in c.attrs.items():
                v = list(v) if isinstance(v, (list, tuple)) else [v]
                f.write(f"ATTR {k} {len(v)} {' '.join(str(int(e)) for e in v)}\n")
            if c.value is not None:
                f.write(f"VALUE f {int(c.value.view(np.uint32)[0]):x}\n" if c.value.dtype == F else f"VALUE i {int(c.value[0])}\n")
            for a in c.inputs:
                ty, w = _words(a)
                f.write(f"IN {ty} {a.ndim} {' '.join(str(d) for d in a.shape)} {w.size} {' '.join(format(int(x), 'x') for x in w)}\n")
            f.write("END\n")


def read_host_results(path):
    out, cid = {}, None
    for line in open(path):
        tok = line.rstrip("\n").split(" ")
        if tok[0] == "CASE":
            cid = tok[1]
        elif tok[0] == "OK":
            rank = int(tok[2])
            shape = [int(d) for d in tok[3:3 + rank]]
            n = int(tok[3 + rank])
            words = np.array([int(w, 16) for w in tok[4 + rank:4 + rank + n]], np.uint32)
            out[cid] = words.view(F if tok[1] == "f" else I32).reshape(shape)
        elif tok[0] == "ERR":
            out[cid] = ("error", tok[1], " ".join(tok[2:]))
        elif tok[0] == "DECLINED":
            out[cid] = "declined"
    return out


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("glue")
    cases = [c for c in T.table() if c.host_program]
    write_host_cases(d / "cases.txt", cases)
    run = subprocess.run([build_glue_hostops_binary(), str(d / "cases.txt"), str(d / "results.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    return cases, read_host_results(d / "results.txt")


def test_host_path_gives_the_rules_bits_over_the_whole_table(host_results):
    cases, got = host_results
    assert len(cases) > 300 and set(got) == {c.id for c in cases}
    wrong = []
    for c in cases:
        g, want = got[c.id], c.want_host
        if isinstance(g, str):  # declined: only what has no host value (8-bit results)
            if not (c.op == "Cast" and c.attrs["to"] in (T.ow.UINT8, T.ow.INT8)):
                wrong.append(f"{c.id}: the host path declined")
        elif isinstance(want, tuple) or isinstance(g, tuple):
            if not (isinstance(g, tuple) and isinstance(want, tuple) and g == want):
                wrong.append(f"{c.id}: {g if isinstance(g, tuple) else 'values of shape ' + str(g.shape)}, the rules say {want if isinstance(want, tuple) else 'values'}")
        elif not R.same_bits(g, want):
            where = np.flatnonzero(g.ravel().view(np.uint32) != want.ravel().view(np.uint32))[:4].tolist() if g.shape == want.shape and g.dtype == want.dtype else None
            wrong.append(f"{c.id}: shape {g.shape} {g.dtype} against {want.shape} {want.dtype}" + (f", first differing elements {where}: {g.ravel()[where]} against {want.ravel()[where]}" if where else ""))
    assert not wrong, f"{len(wrong)} of {len(cases)} cases:\n" + "\n".join(wrong[:60])


def test_python_div_operator_multiplies_by_the_reciprocal_of_a_one_element_divisor():
    from rten_amd import ops
    from rten_amd.recording import RecordingCtx
    from rten_amd.tensor import DeviceTensor
    ctx = RecordingCtx()
    t = lambda *shape: DeviceTensor(ctx, shape, np.float32)

    def launches(op, inputs):
        del ctx.log[:]
        out = op.run(ctx, inputs)
        return out[0], [l for l in ctx.log if l != "rten_hip_malloc"]

    for divisor in (t(), t(1), t(1, 1)):
        y, log = launches(ops.Div(), [t(2, 3), divisor])
        assert log == ["rten_hip_unary_f32", "rten_hip_mul_f32"] and y.shape == (2, 3)
    y, log = launches(ops.Div(), [t(2, 3), t(1, 1, 1)])  # the divisor's rank is the result's: the general multiplication
    assert log == ["rten_hip_unary_f32", "rten_hip_binary_broadcast_f32"] and y.shape == (1, 2, 3)
    assert launches(ops.Div(), [t(2, 3), t(3)])[1] == ["rten_hip_div_f32"]          # more than one element: a division
    assert launches(ops.Div(), [t(), t(2, 3)])[1] == ["rten_hip_binary_broadcast_f32"]  # a one-element DIVIDEND divides
