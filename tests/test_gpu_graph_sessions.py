"""One loaded Graph across changing shapes, captures and plans, on the device: every case of tests/graph_sessions.py through every session, each in ONE
process of tests/cpp/graph_session.cpp (one Context with the pool on, one Graph).  Every action that writes outputs is compared with the node-by-node
interpreter on the binding whose values the feeds then hold -- shape, dtype and bits -- and the plan must show the step kinds the case is there for.

    walk              every binding ascending, descending, shuffled, then the first again: the steps' caches of shape constants (8 copies) and Div's
                      reciprocals evict, the pool's buffers shrink and grow, attention crosses its fused kernel's key limit, the int8 statistics arena and
                      the recurrent kernels see other N / H / W / sequence lengths
    capture_survives  a capture at the first binding outlives eager runs at more than 8 other shapes -- the device copies it reads by address must stay --
                      and takes new values of the same shape
    recapture         capture at one shape, at another, at the first again
    plans_elsewhere   plans autotune chose at the first binding, then a shape-keyed table of non-default plans keyed by the first binding's products, run
                      at every other shape: no plan may change a bit anywhere
    shape_plans_stay  the same table on an untuned graph (a tuned step takes no shape-keyed entry): taken at the first binding, the entries stay on their
                      steps at other shapes, go with a re-plan and are taken again
    outputs_outlive   two held runs at one shape hand out distinct tensors (host-evaluated outputs included: an address comparison), and both still carry
                      their values after runs at every other shape and a scribble over the pool

One process at a time, each under its own time limit, no retries; after a process that ended on a signal or ran out of time, every remaining case fails
without starting another one (the conventions of tests/test_gpu_graph_fuzz.py)."""
import subprocess
import time

import pytest

from tests import graph_sessions as gs
from tests.test_gpu_graph_fuzz import bits_problem, read_safetensors

pytestmark = pytest.mark.gpu

# Measured on an MI355X over every case and session: the slowest process took 0.41 s (attention, plans_elsewhere: one tune at reps 1 and 37 runs; start-up and
# code-object loading dominate, as in tests/test_gpu_graph_fuzz.py).  10x that, rounded up.
TIMEOUT_S = 5.0
_stopped = {"why": None}  # set by the first process that died on a signal or timed out
PAIRS = [(c, s) for c in gs.CASES for s in gs.SESSIONS if s != "outputs_outlive" or c in gs.OUTLIVE_CASES] + [(c, gs.PLANNED_SESSION) for c in gs.PLANNED_CASES]


def run_session(name, kind, tmp, timeout=TIMEOUT_S):
    """(problems, seconds).  Raises RuntimeError after a signal or a timeout (and records it, so that no further process is started)."""
    case = gs.case(name)
    model, script, outputs = gs.write_session(name, kind, tmp)
    probe = gs.build_session_probe()
    t0 = time.monotonic()
    try:
        r = subprocess.run([probe, model, script], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _stopped["why"] = f"{name} [{kind}] did not finish within {timeout} s"
        raise RuntimeError(_stopped["why"])
    seconds = time.monotonic() - t0
    if r.returncode < 0:
        _stopped["why"] = f"{name} [{kind}] ended on signal {-r.returncode}: {r.stderr[-400:]}"
        raise RuntimeError(_stopped["why"])
    problems = []
    kinds = [line[5:].split(":", 1)[0] for line in r.stdout.splitlines() if line.startswith("step ")]
    for want in case.expect["steps"]:
        if want not in kinds:
            problems.append(f"the plan shows no {want} step: {kinds}")
    if r.returncode != 0:
        problems.append(f"exit {r.returncode}: {r.stderr[-600:]}")
    words = gs.read_script(open(script).read())
    for line, path, binding in outputs:
        what = f"line {line} ({' '.join(w.rsplit('/', 1)[-1] for w in words[line - 1])}, binding {binding})"
        try:
            got = read_safetensors(path)
        except OSError:
            if r.returncode == 0:
                problems.append(f"{what}: no output file")
            continue
        want = gs.expected(name, binding)
        if [nm for nm, _ in got] != case.outputs:
            problems.append(f"{what}: outputs {[nm for nm, _ in got]}, expected {case.outputs}")
            continue
        for nm, a in got:
            p = bits_problem(a, want[nm])
            if p:
                problems.append(f"{what}: output {nm}: {p}")
    if kind == "plans_elsewhere" and r.returncode == 0:
        tuned = [line for line in r.stdout.splitlines() if ": tuned " in line]
        if len(tuned) != 1:
            problems.append(f"no report of the tune action: {r.stdout[-300:]}")
        planned = int(r.stdout.rsplit(" steps, ", 1)[1].split()[0]) if " by a shape-keyed plan" in r.stdout else -1
        # a step autotune left a plan on keeps it (the table fills the steps without one): the count is checked only where nothing was tuned
        if gs.gemm_shapes(name) and planned < 0:
            problems.append(f"no report of the shape-keyed plans: {r.stdout[-300:]}")
    if kind == gs.PLANNED_SESSION and r.returncode == 0:
        planned = int(r.stdout.rsplit(" steps, ", 1)[1].split()[0]) if " by a shape-keyed plan" in r.stdout else -1
        if planned != len(gs.gemm_shapes(name)):  # (each case has one step per key)
            problems.append(f"{planned} steps took a shape-keyed entry after the last run at the first binding, expected {len(gs.gemm_shapes(name))}")
    return problems, seconds


@pytest.mark.parametrize("name,kind", PAIRS)
def test_graph_session(name, kind, tmp_path):
    if _stopped["why"]:
        pytest.fail("not run: " + _stopped["why"])
    try:
        problems, seconds = run_session(name, kind, str(tmp_path))
    except RuntimeError as e:
        pytest.fail(str(e))
    print(f"{name} [{kind}]: {seconds:.2f} s")
    assert problems == [], f"{name} [{kind}]:\n  " + "\n  ".join(problems[:40])
