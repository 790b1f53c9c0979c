"""Graph-executor fuzzing on the device: every graph of tests/graph_fuzz.py's corpus through rten_hip_run in three modes -- node by node (--no-fuse),
fused (the default), and captured into a hipGraph and replayed three times on the pool's reused buffers (--graph -n 3) -- against the node-by-node
interpreter: every output's shape, dtype and bits, the number of nodes the plan folded away and the kinds of its fused steps.  The interpreter and
the step counts follow the graph's canonical form (the load-time rewrite of exporter idioms, predicted by tests/fusion_rules.py).

The captured mode checks the folded count only: the CLI prints step kinds in its -t table, which excludes --graph; the plan is made at load, before
any capture, and its kinds are checked in the other two modes.

One process at a time, each under its own time limit, no retries; after a process that ended on a signal or ran out of time, every remaining case
fails without starting another one."""
import functools
import json
import os
import struct
import subprocess
import time

import numpy as np
import pytest

from tests import graph_fuzz as gf
from tests.test_graph_executor import build_cli

pytestmark = pytest.mark.gpu

MODES = {"nofuse": ["--no-fuse", "-t"], "fused": ["-t"], "graph": ["--graph", "-n", "3"]}
# Measured on an MI355X over the whole corpus in all three modes: the slowest process took 0.56 s (a --graph run; start-up and code-object loading
# dominate, the graphs themselves run in microseconds).  10x that, rounded up.
TIMEOUT_S = 6.0
CASE_NAMES = ["hand_" + r.replace("/", "_") for r in gf.ROWS] + [f"seed{s}" for s in range(gf.N_SEEDS)]
_stopped = {"why": None}  # set by the first process that died on a signal or timed out

_NP = {"F32": np.float32, "I32": np.int32, "U8": np.uint8, "I8": np.int8, "I64": np.int64}


@functools.lru_cache(maxsize=4)
def case_by_name(name):
    if name.startswith("seed"):
        return gf.make_case(int(name[4:]))
    return gf.hand_case(gf.ROWS[CASE_NAMES.index(name)])


def read_safetensors(path):
    """[(name, ndarray)] in file order.  Read by hand because a graph may list one value twice in its outputs: the file then carries the name twice,
    and both copies are checked."""
    buf = open(path, "rb").read()
    (n,) = struct.unpack("<Q", buf[:8])
    entries = json.loads(buf[8:8 + n].decode(), object_pairs_hook=list)
    data = buf[8 + n:]
    out = []
    for name, fields in entries:
        if name == "__metadata__":
            continue
        f = dict(fields)
        lo, hi = f["data_offsets"]
        out.append((name, np.frombuffer(data[lo:hi], _NP[f["dtype"]]).reshape(f["shape"])))
    return out


def bits_problem(got, want):
    """None, or how `got` differs from `want` in shape, dtype or bits (NaNs: same positions, payloads not compared)."""
    if tuple(got.shape) != tuple(want.shape):
        return f"shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    if got.dtype != want.dtype:
        return f"dtype {got.dtype}, expected {want.dtype}"
    if got.dtype != np.float32:
        bad = np.flatnonzero(got.ravel() != want.ravel())
        return f"{bad.size} of {got.size} integers differ, first at {bad[0]}: {got.ravel()[bad[0]]} != {want.ravel()[bad[0]]}" if bad.size else None
    g, w = np.ascontiguousarray(got).ravel(), np.ascontiguousarray(want).ravel()
    if not np.array_equal(np.isnan(g), np.isnan(w)):
        return f"NaN positions differ ({int(np.isnan(g).sum())} got, {int(np.isnan(w).sum())} expected)"
    ok = ~np.isnan(w)
    bad = np.flatnonzero(g[ok].view(np.int32) != w[ok].view(np.int32))
    if bad.size:
        return f"{bad.size} of {g.size} elements differ in their bits, first at {bad[0]}: {g[ok][bad[0]]!r} != {w[ok][bad[0]]!r} (max abs diff {np.abs(g[ok] - w[ok]).max():.3e})"
    return None


def parse_plan(stdout):
    """(steps, folded, [(kind, count)]) from the CLI's `Plan:` line and, with -t, its per-operator table."""
    steps = folded = None
    kinds, in_table = [], False
    for line in stdout.splitlines():
        if line.startswith("Plan: "):
            words = line.split()
            steps, folded = int(words[1]), int(words[3].lstrip("("))
        elif "Operator timing" in line:
            in_table = True
        elif in_table and line.startswith("    "):
            left = line.rsplit("ms", 1)[0].rsplit(None, 2)  # "<kind> x<count> <t>"
            kinds.append((left[0].strip(), int(left[1].lstrip("x"))))
        elif in_table:
            in_table = False
    return steps, folded, kinds


def check_mode(case, mode, tmp, timeout=TIMEOUT_S):
    """Runs `case` in one mode, once per input binding.  Returns (problems, seconds of the slowest process); raises RuntimeError after a signal or a
    timeout (and records it, so that no further process is started)."""
    from safetensors.numpy import save_file
    fused = mode != "nofuse"
    problems, slowest = [], 0.0
    model = os.path.join(tmp, f"{case.name}.onnx")
    with open(model, "wb") as f:
        f.write(case.onnx)
    for k, binding in enumerate(case.bindings):
        xin, yout = os.path.join(tmp, f"{case.name}.{k}.in.safetensors"), os.path.join(tmp, f"{case.name}.{k}.{mode}.out.safetensors")
        save_file({name: np.ascontiguousarray(a) for name, a in binding.items()}, xin)
        if os.path.exists(yout):
            os.remove(yout)
        t0 = time.monotonic()
        try:
            r = subprocess.run([build_cli(), *MODES[mode], "--inputs", xin, "--save-outputs", yout, model], capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            _stopped["why"] = f"{case.name} [{mode}] did not finish within {timeout} s"
            raise RuntimeError(_stopped["why"])
        slowest = max(slowest, time.monotonic() - t0)
        if r.returncode < 0:
            _stopped["why"] = f"{case.name} [{mode}] ended on signal {-r.returncode}: {r.stderr[-400:]}"
            raise RuntimeError(_stopped["why"])
        steps, folded, kinds = parse_plan(r.stdout)
        want_folded = case.expect["folded"] if fused else 0
        if folded != want_folded:
            problems.append(f"binding {k}: the plan folded {folded} nodes, expected {want_folded}")
        if steps is not None and folded is not None and not fused and steps != case.expect["canonical_nodes"]:  # one step per node of the canonical form
            problems.append(f"binding {k}: --no-fuse planned {steps} steps for {case.expect['canonical_nodes']} canonical nodes ({len(case.nodes)} as written)")
        error = (case.expect["error"] or {}).get("fused" if fused else "nofuse")
        if error:
            if r.returncode != 1 or error not in r.stderr:
                problems.append(f"binding {k}: expected a clean exit 1 with {error!r}, got exit {r.returncode}: {r.stderr[-300:]}")
            continue
        if r.returncode != 0:
            problems.append(f"binding {k}: exit {r.returncode}: {r.stderr[-400:]}")
            continue
        if mode != "graph":  # (--timing and --graph exclude each other: the captured mode checks the folded count only)
            got_kinds = sorted(kd for kd, n in kinds for _ in range(n) if gf.is_fused_kind(kd))
            want_kinds = case.expect["kinds"] if fused else []
            if got_kinds != want_kinds:
                problems.append(f"binding {k}: fused step kinds {got_kinds}, expected {want_kinds}")
        want = gf.evaluate(case, k, fused=fused)
        got = read_safetensors(yout)
        if [name for name, _ in got] != case.outputs:
            problems.append(f"binding {k}: outputs {[name for name, _ in got]}, expected {case.outputs}")
            continue
        for name, a in got:
            p = bits_problem(a, want[name])
            if p:
                problems.append(f"binding {k}: output {name} ({gf_producer(case, name)}): {p}")
    return problems, slowest


def check_outputs_outlive_run(case, tmp, timeout=TIMEOUT_S, probe=None):
    """The fused plan through the probe program: the outputs must still carry the interpreter's bits after the pool has been reused."""
    from safetensors.numpy import save_file
    model, xin, yout = (os.path.join(tmp, f"{case.name}.{x}") for x in ("onnx", "in.safetensors", "probe.safetensors"))
    with open(model, "wb") as f:
        f.write(case.onnx)
    save_file({name: np.ascontiguousarray(a) for name, a in case.inputs.items()}, xin)
    try:
        r = subprocess.run([probe or gf.build_outlive_probe(), model, xin, yout], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _stopped["why"] = f"{case.name} [probe] did not finish within {timeout} s"
        raise RuntimeError(_stopped["why"])
    if r.returncode < 0:
        _stopped["why"] = f"{case.name} [probe] ended on signal {-r.returncode}: {r.stderr[-400:]}"
        raise RuntimeError(_stopped["why"])
    if r.returncode != 0:
        return [f"exit {r.returncode}: {r.stderr[-400:]}"]
    want, got = gf.evaluate(case, 0, fused=True), read_safetensors(yout)
    if [name for name, _ in got] != case.outputs:
        return [f"outputs {[name for name, _ in got]}, expected {case.outputs}"]
    return [f"output {name} ({gf_producer(case, name)}): {p}" for name, a in got for p in [bits_problem(a, want[name])] if p]


def gf_producer(case, name):
    for n in case.nodes:
        if name in n["outputs"]:
            return n["op"]
    return "graph input" if name in case.inputs else "initializer"


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_graph_fuzz(name, mode, tmp_path):
    if _stopped["why"]:
        pytest.fail("not run: " + _stopped["why"])
    case = case_by_name(name)
    try:
        problems, _ = check_mode(case, mode, str(tmp_path))
    except RuntimeError as e:
        pytest.fail(str(e))
    assert problems == [], f"{name} [{mode}] rows {case.expect['rows']}:\n  " + "\n  ".join(problems)


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n.startswith("hand_views_")])
def test_outputs_own_their_storage_after_the_run(name, tmp_path):
    """A view, a graph input, an initializer or a value listed twice, returned as an output, is a copy: it survives the reuse of the run's buffers."""
    if _stopped["why"]:
        pytest.fail("not run: " + _stopped["why"])
    case = case_by_name(name)
    try:
        problems = check_outputs_outlive_run(case, str(tmp_path))
    except RuntimeError as e:
        pytest.fail(str(e))
    assert problems == [], f"{name}:\n  " + "\n  ".join(problems)
