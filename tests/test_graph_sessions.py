"""The shape-polymorphic cases and sessions of tests/graph_sessions.py, checked without a device: determinism, the C++ loader reads every case, the f32
interpreter agrees with an independent float64 evaluation on every binding, the scripts round-trip, the conditions that make the sessions mean something
hold, and the session probe (tests/cpp/graph_session.cpp) compiles -- its host-only half also under AddressSanitizer / UndefinedBehaviorSanitizer."""
import subprocess

import numpy as np
import pytest

from tests import graph_fuzz as gf
from tests import graph_sessions as gs
from tests.test_graph_executor import run_cli

NAMES = list(gs.CASES)


def test_same_case_same_bytes():
    for name in NAMES:
        a, b = gs.CASES[name](), gs.CASES[name]()
        assert a.onnx == b.onnx and a.outputs == b.outputs and a.expect == b.expect and len(a.bindings) == len(b.bindings), name
        for x, y in zip(a.bindings, b.bindings):
            assert list(x) == list(y) and all(np.array_equal(x[k], y[k]) for k in x), name
    assert len({gs.case(n).onnx for n in NAMES}) == len(NAMES)
    assert not set(gs.case(n).name for n in NAMES) & {c.name for c in (gf.hand_case(r) for r in gf.ROWS)}  # beside the corpus, not in it


@pytest.mark.parametrize("name", NAMES)
def test_case_declares_dynamic_axes_and_binds_them_at_ten_shapes(name):
    c = gs.case(name)
    assert any(isinstance(d, str) for _, dims in c.input_specs for d in dims), name
    assert len(c.bindings) >= 11
    shapes = [tuple(b[k].shape for k, _ in c.input_specs) for b in c.bindings]
    assert len(set(shapes[:-1])) == len(shapes) - 1 >= 10, shapes                       # pairwise different ...
    assert shapes[-1] == shapes[0] and any(not np.array_equal(c.bindings[0][k], c.bindings[-1][k]) for k in c.bindings[0])  # ... then the first again, other values
    for b in c.bindings:
        for k, dims in c.input_specs:
            assert all(isinstance(d, str) or d == s for d, s in zip(dims, b[k].shape)), (name, k, dims, b[k].shape)
    for k in range(len(c.bindings)):
        for vname, v in gs.expected(name, k).items():
            assert v.size <= gf.MAX_ELEMS, (name, k, vname, v.shape)
    assert c.expect["steps"] and all(isinstance(s, str) and s for s in c.expect["steps"])  # the plan's expected kinds are named


def test_cases_reach_the_steps_they_are_there_for():
    """From the node lists: the operators behind the expected step kinds are in the graphs, attention crosses the fused kernel's key limit of 128 inside one
    case, the recurrent case stands on both sides of the 5-step weight prepacking, and shape_scalars returns host-evaluated values as graph outputs."""
    ops = {n: [x["op"] for x in gs.case(n).nodes] for n in NAMES}
    assert ops["int8_chain"].count("DynamicQuantizeLinear") == 2 and ops["int8_chain"].count("ConvInteger") == 2
    assert {"GRU", "LSTM"} <= set(ops["rnn_dynamic"]) and {"Equal", "Where", "Expand", "Softmax", "LayerNormalization"} <= set(ops["attention"])
    seqs = [b[gs.case("attention").input_specs[0][0]].shape[1] for b in gs.case("attention").bindings]
    assert {1, 2, 7, 16, 17, 33, 64, 100, 128, 129, 130} <= set(seqs)
    assert {s for s, _ in gs.RNN_SHAPES} == set(range(1, 10)) and {n for _, n in gs.RNN_SHAPES} == {1, 2, 3}
    assert {1, 15, 16, 17, 257} <= set(gs.SCALAR_LENGTHS) and len(set(gs.SCALAR_LENGTHS)) == 10
    c = gs.case("shape_scalars")
    made_by = {o: n["op"] for n in c.nodes for o in n["outputs"]}
    assert sorted(made_by[o] for o in c.outputs) == ["Cast", "Concat", "Div", "Mul", "Shape"]
    assert [str(gs.expected("shape_scalars", 0)[o].dtype) for o in c.outputs] == ["float32", "int32", "int32", "float32", "float32"]
    # no host-evaluated value is a device Gather / Scatter index
    for n in NAMES:
        c = gs.case(n)
        host = _host_evaluated(c)
        for node in c.nodes:
            if node["op"].startswith(("Gather", "Scatter")) and node["inputs"][0] not in host:
                assert not set(node["inputs"][1:]) & (host - set(c.inits)), (n, node["op"])


def _host_evaluated(c):
    """Names whose values depend only on input SHAPES and constants: what the executor evaluates on the host."""
    host = set(c.inits)
    for n in c.nodes:
        if n["op"] == "Shape" or (n["op"] in gf.LAYOUT_OPS + gf.GLUE_OPS + ("Cast", "Add", "Sub", "Mul", "Div") and all(s in host for s in n["inputs"] if s)):
            host.update(o for o in n["outputs"] if o)
    return host


@pytest.mark.parametrize("name", NAMES)
def test_sessions_see_more_host_values_than_a_step_caches(name):
    """A host-evaluated step keeps 8 device copies.  Every such value a session relies on takes at least 9 distinct values over the bindings -- so a walk
    evicts, and the runs between a capture and its last replay push the captured copy out of the cache -- and every value named is indeed host-evaluated."""
    c = gs.case(name)
    assert set(c.expect["host"]) <= _host_evaluated(c) - set(c.inits)
    assert c.expect["host"] or name == "int8_chain"  # (its state across shapes is the statistics arena, not shape arithmetic)
    for h in c.expect["host"]:
        seen = {(gs.expected(name, k)[h].shape, gs.expected(name, k)[h].tobytes()) for k in range(len(c.bindings))}
        assert len(seen) >= 9, (name, h, len(seen))
        between = {gs.expected(name, k)[h].tobytes() for words, k in gs.session(name, "capture_survives")[2:-3]}
        assert len(between) >= 9 and gs.expected(name, 0)[h].tobytes() not in between, (name, h)
    if name == "shape_scalars":  # ... and Div's reciprocal cache: the divisor itself
        divisor = [n["inputs"][1] for n in c.nodes if n["op"] == "Div"][0]
        assert divisor in c.expect["host"] and gs.expected(name, 0)[divisor].size == 1


def test_cpp_loader_parses_every_case(tmp_path):
    for name in NAMES:
        c = gs.case(name)
        p = tmp_path / "m.onnx"
        p.write_bytes(c.onnx)
        out = run_cli("--parse-only", str(p), timeout=60)
        assert out.returncode == 0, (name, out.stderr)
        assert f"{len(c.nodes)} nodes, {len(c.inits)} initializers" in out.stdout, (name, out.stdout)
        assert "canonical form" not in out.stdout, (name, out.stdout)
        for iname, _ in c.input_specs:
            assert f"input  {iname}:" in out.stdout, (name, iname)


@pytest.mark.parametrize("name", NAMES)
def test_interpreter_against_independent_float64(name):
    """Every float value of every binding, f32 interpreter against float64, under test_graph_fuzz_oracle's bound and tie rules: deviation =
    |f32 - f64| / (1 + |f64|) <= gf.F64_BOUND (8.5e-6, set there from the committed corpus); integer values are compared exactly where the float64
    decision is not within the same margin of a tie.  Both the node-by-node values and those of the fused expectation the sessions compare with."""
    c = gs.case(name)
    worst, worst_at, ints, skipped = 0.0, None, 0, 0
    for k in range(len(c.bindings)):
        teacher = gf.evaluate(c, k, fused=False)
        v64, ties = gf.evaluate64(c, k, teacher=teacher)
        for which, vals in (("nodes", teacher), ("fused", gs.expected(name, k))):
            for n in c.nodes:
                for o in n["outputs"]:
                    if not o or o not in vals:
                        continue
                    got = vals[o]
                    if got.dtype == np.float32:
                        want = v64[o]
                        assert got.shape == want.shape and want.dtype == np.float64, (name, k, n["op"], o, got.shape, want.shape)
                        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, k, n["op"], o)
                        fin = np.isfinite(want)
                        assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), (name, k, n["op"], o)
                        if fin.any():
                            d = float((np.abs(got[fin].astype(np.float64) - want[fin]) / (1.0 + np.abs(want[fin]))).max())
                            if d > worst:
                                worst, worst_at = d, (k, which, n["op"], o)
                    elif which == "nodes" and o + "#f64" in v64:
                        want = v64[o + "#f64"]
                        assert got.shape == want.shape, (name, k, n["op"], o)
                        tie = np.broadcast_to(ties.get(o, np.zeros((), bool)), got.shape)
                        ints += got.size
                        skipped += int(tie.sum())
                        assert np.array_equal(got[~tie].astype(np.int64), want[~tie].astype(np.int64)), (name, k, n["op"], o)
                    elif which == "nodes":  # layout operators on integers (Shape, Gather, Concat, Slice ...): exact in any precision
                        assert np.array_equal(got.astype(np.int64), np.asarray(v64[o]).astype(np.int64)), (name, k, n["op"], o)
    print(f"{name}: worst f32 / float64 deviation {worst:.3e} at {worst_at}; {skipped} of {ints} integer elements near a tie")
    assert worst <= gf.F64_BOUND, (name, worst, worst_at)
    assert skipped <= 0.01 * max(ints, 1), (name, skipped, ints)


@pytest.mark.parametrize("kind", gs.SESSIONS + (gs.PLANNED_SESSION,))
def test_scripts_round_trip(kind, tmp_path):
    for name in NAMES if kind != gs.PLANNED_SESSION else gs.PLANNED_CASES:
        d = tmp_path / name
        d.mkdir()
        model, script, outputs = gs.write_session(name, kind, str(d))
        text = open(script).read()
        actions = gs.read_script(text)
        assert gs.format_script(actions) == text and gs.read_script(gs.format_script(actions)) == actions
        want = gs.session(name, kind)
        assert [a[0] for a in actions] == [w[0][0] for w in want] and len(actions) <= 45
        assert [line for line, _, _ in outputs] == [i + 1 for i, (w, _) in enumerate(want) if "@" in w]
        assert [b for _, _, b in outputs] == [b for w, b in want if "@" in w]
        assert open(model, "rb").read() == gs.case(name).onnx
    assert gs.read_script("run a b # comment\n\n  # only a comment\nreplay  c\n") == [["run", "a", "b"], ["replay", "c"]]


def test_sessions_do_what_their_names_say():
    n = len(gs.case("conv_reshape_matmul").bindings)
    order = gs.walk_order(n)
    assert order[:n] == list(range(n)) and order[n:2 * n] == list(range(n - 1, -1, -1)) and sorted(order[2 * n:3 * n]) == list(range(n)) and order[3 * n:] == [0]
    assert order[2 * n:3 * n] not in (order[:n], order[n:2 * n]) and gs.walk_order(n) == order
    verbs = lambda kind: [w[0] for w, _ in gs.session("conv_reshape_matmul", kind)]
    assert verbs("capture_survives") == ["capture", "replay"] + ["run"] * (n - 2) + ["replay", "refill", "replay"]
    assert verbs("recapture") == ["capture", "replay"] * 3 and [b for _, b in gs.session("attention", "recapture")] == [0, 0, 5, 5, 0, 0]
    assert verbs("plans_elsewhere") == ["tune"] + ["run"] * (3 * n + 1) + ["shape-plans", "run", "run", "run"]
    assert [b for _, b in gs.session("conv_reshape_matmul", "plans_elsewhere")[-3:]] == [1, 0, 1]
    assert verbs("outputs_outlive") == ["hold", "hold", "distinct"] + ["run"] * (n - 1) + ["read", "read"]
    # the shape-keyed table is keyed by the FIRST binding's own products and names no default plan
    assert gs.gemm_shapes("conv_reshape_matmul") == ["gemm:1x144x10"] and gs.gemm_shapes("attention") == ["gemm:1x128x128", "gemm:1x128x384"]
    assert all(p[0] >= 0 for p in gs.SHAPE_PLANS)
    assert gs.PLANNED_CASES == tuple(nm for nm in NAMES if gs.gemm_shapes(nm))
    assert verbs(gs.PLANNED_SESSION) == ["shape-plans", "run", "run", "run", "run", "run", "shape-plans", "run", "run"]
    assert [b for _, b in gs.session("attention", gs.PLANNED_SESSION)] == [None, 1, 0, 1, 10, 0, None, 1, 0]


def test_probe_compiles_and_its_host_half_is_clean_under_sanitizers(tmp_path):
    """-Wall -Werror for the probe itself; then the same source under -fsanitize=address,undefined as a stand-alone program, run on a real session's files in
    its --check-script mode (script parser, plan table, Safetensors reader and writer: everything of the probe that needs no device) and on malformed scripts."""
    gs.build_session_probe()
    san = gs.build_session_probe(sanitize=True)
    model, script, outputs = gs.write_session("attention", "plans_elsewhere", str(tmp_path))
    r = subprocess.run([san, "--check-script", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"script ok: {len(gs.session('attention', 'plans_elsewhere'))} actions" in r.stdout, r.stdout[-800:] + r.stderr[-2000:]
    from tests.test_gpu_graph_fuzz import read_safetensors
    echoed = dict(read_safetensors(outputs[0][1]))  # `run` echoes its inputs through the reader and the writer
    first = gs.case("attention").bindings[outputs[0][2]]
    assert set(echoed) == set(first) and all(np.array_equal(echoed[k], first[k]) and echoed[k].dtype == first[k].dtype for k in first)
    for text, needle in (("walk b0 out\n", "line 1: unknown action walk"), ("run b0\n", "line 1: run takes 2 operand(s)"),
                         ("# nothing\nrun " + str(tmp_path / "missing.safetensors") + " x\n", "line 2 (run): safetensors: cannot open")):
        bad = tmp_path / "bad.txt"
        bad.write_text(text)
        r = subprocess.run([san, "--check-script", str(bad)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and needle in r.stderr and "Sanitizer" not in r.stderr, (text, r.stderr[-2000:])
    short = tmp_path / "short.safetensors"
    short.write_bytes(open(str(tmp_path / "b0.safetensors"), "rb").read()[:40])
    bad.write_text(f"tune {short}\n")
    r = subprocess.run([san, "--check-script", str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "line 1 (tune): safetensors:" in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
