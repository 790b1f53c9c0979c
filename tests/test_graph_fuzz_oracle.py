"""The graph fuzzer's generator and interpreter (tests/graph_fuzz.py), checked without a device: determinism, the C++ loader reads every graph,
every row of the motif / spoiler table occurs, and the f32 interpreter agrees with an independent float64 evaluation."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

from tests import graph_fuzz as gf
from tests.test_graph_executor import run_cli


@pytest.fixture(scope="module")
def corpus():
    return gf.corpus()


def test_same_seed_same_bytes():
    for seed in (0, 1, 17, gf.N_SEEDS - 1):
        a, b = gf.make_case(seed), gf.make_case(seed)
        assert a.onnx == b.onnx and a.outputs == b.outputs and a.expect == b.expect
        for k in a.inputs:
            assert np.array_equal(a.inputs[k], b.inputs[k])
    assert gf.make_case(1).onnx != gf.make_case(2).onnx
    row = gf.ROWS[3]
    assert gf.hand_case(row).onnx == gf.hand_case(row).onnx


def test_corpus_shape(corpus):
    assert len(corpus) == len(gf.ROWS) + gf.N_SEEDS and gf.N_SEEDS >= 64
    assert len({c.name for c in corpus}) == len(corpus)
    for k, c in enumerate(corpus[len(gf.ROWS):]):
        assert 6 <= len(c.nodes) <= (30 if k < gf.OLD_SEEDS else gf.MAX_NODES_NEW), (c.name, len(c.nodes))
    vals_seen = 0
    for c in corpus:
        for k in range(len(c.bindings)):
            try:
                vals = gf.evaluate(c, k, fused=False)
            except gf.ExpectedError:
                continue
            for name, v in vals.items():
                assert v.size <= gf.MAX_ELEMS, (c.name, name, v.shape)
                vals_seen += 1
    assert vals_seen > 2000


def test_every_table_row_occurs(corpus):
    """Computed from Case.expect: a row dropped from the generator (or from ROWS' source tables) fails here."""
    table = {"conv": 23, "matmul": 24, "gemm": 7, "add_ln": 6, "add_softmax": 6, "views": 16, "int8": 6, "shape": 1, "idiom": 40, "attention": 20, "norm_act": 21, "qdq": 9}
    assert collections.Counter(r.split("/")[0] for r in gf.ROWS) == table
    hand = collections.Counter(r for c in corpus[:len(gf.ROWS)] for r in c.expect["rows"])
    rand = collections.Counter(r for c in corpus[len(gf.ROWS):] for r in c.expect["rows"])
    assert [r for r in gf.ROWS if hand[r] != 1] == []                                       # one minimal graph per row
    assert [r for r in gf.ROWS if not rand[r] and r not in gf.HAND_ONLY_ROWS] == []         # and each motif row inside a random graph too
    new = collections.Counter(r for c in corpus[len(gf.ROWS) + gf.OLD_SEEDS:] for r in c.expect["rows"])
    assert [r for r in gf.NEW_ROWS if not new[r]] == []                                     # the rows added later: among the seeds from 64 on
    assert not any(r in gf.NEW_ROWS for c in corpus[len(gf.ROWS):len(gf.ROWS) + gf.OLD_SEEDS] for r in c.expect["rows"])
    # the spoilers the table names, by what they must do to the plan
    by_row = {c.expect["rows"][0]: c.expect for c in corpus[:len(gf.ROWS)]}
    must_not_fuse = ["conv/res_after", "conv/add_same", "conv/out_second_reader", "conv/out_is_graph_output", "matmul/div_left", "matmul/bias_1xn",
                     "matmul/bias_nonconst", "matmul/read_twice", "add_ln/axis_other", "add_ln/add_out_is_scale", "add_ln/add_is_output", "add_softmax/other_axis"]
    must_not_fuse += ["idiom/" + v for v in gf.IDIOM_MUST_NOT_FUSE] + ["norm_act/in_follower_read_twice", "norm_act/bn_out_is_output", "norm_act/logsoftmax_relu"]
    must_not_fuse += ["attention/" + v for v in gf.ATTENTION_SPOILED]
    assert by_row["attention/v_head_count_differs"]["error"] == {"fused": gf.PARTIAL_BROADCAST_ERROR, "nofuse": gf.PARTIAL_BROADCAST_ERROR, "device_only": True}
    for v in gf.ATTENTION_FUSING:
        assert by_row["attention/" + v]["kinds"] in (["MultiHeadSdpa"], ["FusedMatMul(QKV)", "MultiHeadSdpa(QKV column blocks)"]) and by_row["attention/" + v]["folded"] >= 11, v
    must_not_fuse += ["qdq/zero_points_differ", "qdq/scales_differ", "qdq/codes_read_twice", "qdq/codes_is_output", "qdq/runtime_scale", "qdq/dql_over_initializers"]
    assert sorted(k for r, e in by_row.items() if r.startswith("norm_act/") for k in e["kinds"]) == sorted(n + "+" + a for n in ("InstanceNormalization", "BatchNormalization")
                                                                                                        for a in ("Relu",) + gf.ACT_KINDS)
    assert [by_row["qdq/" + v]["kinds"] for v in ("pair_u8", "pair_i8", "pair_per_axis")] == [["QuantizeLinear+DequantizeLinear"]] * 3
    assert by_row["qdq/dql_over_initializers"]["folded_dequantize"] == (1, 7) and dict(by_row["qdq/dql_over_initializers"]["canonical"]).get("DequantizeLinear") is None
    for r in must_not_fuse:
        assert by_row[r]["folded"] == 0 and by_row[r]["kinds"] == [], r
    # the idiom rows, by what the reference's rules make of them: a spoiled idiom stays as written, every other one becomes its one operator
    for v in gf.IDIOM_VARIANTS:
        e = by_row["idiom/" + v]
        ops = dict(e["canonical"] or [])
        fused_op = "Gelu" if v.startswith("gelu") or v == "constant_node" else "Silu" if v.startswith("silu") else "Swish" if v.startswith("swish") else "LayerNormalization"
        if v in gf.IDIOM_MUST_NOT_FUSE:
            assert e["canonical"] is None, v
        else:
            assert ops.get(fused_op) == 1 and not set(ops) & {"Erf", "Sigmoid", "Sqrt", "Pow", "ReduceMean", "Constant"}, (v, ops)
    assert by_row["conv/add_is_output_relu_after"] == dict(by_row["conv/add_is_output_relu_after"], folded=1, kinds=["Conv+Add"])
    assert by_row["conv/two_convs_one_add"]["kinds"] == ["Conv+Add+Relu"] and by_row["matmul/div_then_mul"]["folded"] == 1
    assert by_row["matmul/bias_len_mismatch"]["error"] == {"fused": "Cannot broadcast bias to output shape", "nofuse": None}
    assert sorted(k.split("+")[1] for r, e in by_row.items() if r.startswith("conv/act_") for k in e["kinds"]) == sorted(gf.ACT_KINDS)
    # the glue of the later operator families: every pick occurs among the seeds of the extended table
    later = collections.Counter(n["op"] for c in corpus[len(gf.ROWS) + gf.OLD_SEEDS:] for n in c.nodes)
    for op in ("InstanceNormalization", "LogSoftmax", "Pad", "Neg", "Abs", "Sqrt", "Exp", "Max", "Mean", "ReduceL2", "ReduceLogSumExp", "ReduceMax", "GlobalMaxPool", "CumSum",
               "Trilu", "Tile", "GatherElements", "DepthToSpace", "Resize"):
        assert later[op] >= 1, op
    assert {n["attrs"].get("mode") for c in corpus[len(gf.ROWS) + gf.OLD_SEEDS:] for n in c.nodes if n["op"] == "Pad"} == {"constant", "reflect"}
    assert sum(1 for c in corpus if len(c.bindings) == 2) >= 1                              # the dynamic axis bound at two sizes
    assert sum(1 for c in corpus if len(c.outputs) != len(set(c.outputs))) >= 1             # an output listed twice
    assert sum(1 for c in corpus if set(c.outputs) & set(c.inputs)) >= 1                    # a graph input returned as an output


def test_old_corpus_has_not_moved():
    """The graphs of the first table and the first 64 seeds are byte-identical to the ones recorded before the table was extended."""
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_fuzz_corpus.json")))
    cases = [gf.hand_case(r) for r in gf.OLD_ROWS] + [gf.make_case(s) for s in range(gf.OLD_SEEDS)]
    assert len(cases) == len(want) == 153
    assert [c.name for c in cases if hashlib.sha256(c.onnx).hexdigest() != want[c.name]] == []


def test_cpp_loader_parses_every_graph(corpus, tmp_path):
    """... and the load-time canonicalisation (Constant nodes, Silu / Swish / Gelu / LayerNormalization idioms) leaves exactly the operators that the
    reference's rules (tests/fusion_rules.py) predict: no canonical form line where they rewrite nothing, the predicted operator counts elsewhere."""
    assert sum(1 for c in corpus if c.expect["canonical"]) >= 40 and sum(1 for c in corpus[:len(gf.OLD_ROWS)] if c.expect["canonical"]) == 0
    for c in corpus:
        p = tmp_path / "m.onnx"
        p.write_bytes(c.onnx)
        out = run_cli("--parse-only", str(p), timeout=60)
        assert out.returncode == 0, (c.name, out.stderr)
        assert f"{len(c.nodes)} nodes, {len(c.inits)} initializers" in out.stdout, (c.name, out.stdout)
        line = [l for l in out.stdout.splitlines() if "canonical form (" in l]
        if c.expect["canonical"] is None:
            assert line == [], (c.name, out.stdout)
        else:
            assert len(line) == 1, (c.name, c.expect["rows"], c.expect["canonical"], out.stdout)
            words = line[0].split("nodes:")
            got = sorted((k, int(v.lstrip("x"))) for k, v in zip(words[1].split()[::2], words[1].split()[1::2]))
            assert int(words[0].split()[-1]) == c.expect["canonical_nodes"] and got == c.expect["canonical"], (c.name, c.expect["rows"], got, c.expect["canonical"])
        fd = c.expect["folded_dequantize"]
        assert ("constant DequantizeLinear folded" in out.stdout) == (fd is not None), (c.name, out.stdout)
        if fd:
            assert f"canonical form: {fd[0]} constant DequantizeLinear folded into float32 initializers ({fd[1]} initializers remain)" in out.stdout, (c.name, fd, out.stdout)
        for name, dims in c.input_specs:
            assert f"input  {name}:" in out.stdout, (c.name, name)


def test_fused_and_unfused_expectations_differ_only_where_the_case_says(corpus):
    for c in corpus:
        if c.expect["error"] and c.expect["error"].get("device_only"):  # a stated limit of the device path: the reference's rules run the graph in both modes
            a, b = gf.evaluate(c, 0, fused=True), gf.evaluate(c, 0, fused=False)
            assert all(np.array_equal(a[o], b[o], equal_nan=True) for o in c.outputs) or c.expect["modes_differ"], c.name
            continue
        if c.expect["error"]:
            with pytest.raises(gf.ExpectedError, match=c.expect["error"]["fused"]):
                gf.evaluate(c, 0, fused=True)
            gf.evaluate(c, 0, fused=False)
            continue
        a, b = gf.evaluate(c, 0, fused=True), gf.evaluate(c, 0, fused=False)
        same = all(np.array_equal(a[o], b[o], equal_nan=True) for o in c.outputs)
        assert same or c.expect["modes_differ"], c.name
    assert sum(1 for c in corpus if c.expect["modes_differ"]) >= 10


def test_interpreter_against_independent_float64(corpus):
    """Every float value of every graph, f32 oracle against float64: deviation = |f32 - f64| / (1 + |f64|).

    Measured over this corpus (the 96 seeds and every row), from the interpreter and evaluate64 alone: worst deviation 5.83e-6 (seed90, a MatMul of an
    attention row; before the table was extended it was 2.13e-6, matmul/div_right_np2); the values that the fused
    expectation computes differently (FusedMatMul with alpha, the bias position) deviate by 1.02e-6 at most.  The bound is 4x the worst,
    gf.F64_BOUND = 2.34e-5 -- the corpus is fixed, only libm varies.  The result of an idiom of gf.IDIOM_OFF_NOMINAL, and what is computed from
    it, is not compared (the nodes spell another function than the one the reference runs): that result must deviate by MORE than the bound.  Integer outputs (u8 codes and zero points, ArgMax / TopK indices) are compared
    where the float64 decision is not within the same bound of a tie; fewer than 1% of them may be left out on that ground."""
    worst, worst_at, worst_fused = 0.0, None, 0.0
    ints = skipped = 0
    off_nominal = [c for c in corpus if c.expect["off_nominal"]]
    assert len(off_nominal) >= 2 * len(gf.IDIOM_OFF_NOMINAL)
    compared_in_off_nominal = 0
    for c in corpus:
        for k in range(len(c.bindings)):
            teacher = gf.evaluate(c, k, fused=False)
            with np.errstate(all="ignore"):
                v64, ties = gf.evaluate64(c, k, teacher=teacher)
            # gf.IDIOM_OFF_NOMINAL: the idiom's result must differ measurably from the nodes as written; it and whatever is computed from it are not compared
            tainted = set(c.expect["off_nominal"] or [])
            for o in tainted:
                w = v64[o]
                assert np.isnan(w).any() or float((np.abs(teacher[o] - w) / (1.0 + np.abs(w))).max()) > gf.F64_BOUND, (c.name, o)
            for n in c.nodes:
                if tainted & set(n["inputs"]):
                    tainted |= set(n["outputs"])
            for n in c.nodes:
                for o in n["outputs"]:
                    if not o or o not in teacher or o in tainted:  # (an interior value of a fused idiom does not exist for the interpreter)
                        continue
                    compared_in_off_nominal += bool(c.expect["off_nominal"])
                    got = teacher[o]
                    if got.dtype == np.float32:
                        want = v64[o]
                        assert got.shape == want.shape and want.dtype == np.float64, (c.name, n["op"], o)
                        assert np.array_equal(np.isnan(got), np.isnan(want)), (c.name, n["op"], o)
                        fin = np.isfinite(want)
                        assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), (c.name, n["op"], o)
                        if fin.any():
                            d = float((np.abs(got[fin].astype(np.float64) - want[fin]) / (1.0 + np.abs(want[fin]))).max())
                            if d > worst:
                                worst, worst_at = d, (c.name, n["op"], o)
                    elif o + "#f64" in v64:
                        want = v64[o + "#f64"]
                        assert got.shape == want.shape, (c.name, n["op"], o)
                        tie = np.broadcast_to(ties.get(o, np.zeros((), bool)), got.shape)
                        ints += got.size
                        skipped += int(tie.sum())
                        assert np.array_equal(got[~tie].astype(np.int64), want[~tie].astype(np.int64)), (c.name, n["op"], o)
            # ... and the interpreter's arithmetic-changing rules (FusedMatMul with alpha, the bias position): every float value of the FUSED
            # expectation against the same float64 values, same bound
            try:
                fused = gf.evaluate(c, k, fused=True)
            except gf.ExpectedError:
                continue
            for o, got in fused.items():
                if got.dtype != np.float32 or o not in v64 or o in tainted or np.array_equal(got, teacher[o], equal_nan=True):  # (only what the rules changed)
                    continue
                want = v64[o]
                assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (c.name, "fused", o)
                fin = np.isfinite(want)
                if fin.any():
                    d = float((np.abs(got[fin].astype(np.float64) - want[fin]) / (1.0 + np.abs(want[fin]))).max())
                    worst_fused = max(worst_fused, d)
                    if d > worst:
                        worst, worst_at = d, (c.name, "fused", o)
    print(f"worst deviation of the fused expectation {worst_fused:.3e}")
    assert worst_fused > 0.0 and compared_in_off_nominal >= 4 * len(off_nominal)  # (a graph that carries an off-nominal idiom is compared up to it: at least the four nodes that shape its operand)
    print(f"worst f32 / float64 deviation {worst:.3e} at {worst_at}; {skipped} of {ints} integer elements near a tie")
    assert worst <= gf.F64_BOUND, (worst, worst_at)  # measured 5.83e-6, bound 4x = 2.34e-5
    assert ints > 1000 and skipped < 0.01 * ints, (skipped, ints)
