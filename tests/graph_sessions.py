"""Shape-polymorphic graphs and the sessions that run ONE loaded Graph over them (tests/cpp/graph_session.cpp): the way the executor is meant to be used
-- loaded once, then run at changing input shapes, captured, replayed, re-captured and re-planned.

A case is a tests/graph_fuzz.py `Case` built with its `Builder`, with dynamic axes and 11 or more bindings: at least 10 pairwise different input shapes and a
last one that repeats the FIRST shape with other values (what `refill` writes into a captured graph's feeds).  Beyond graph_fuzz's expectations a case
records
    expect["steps"]   step kinds its plan must show (a case must not silently stop reaching the step it is there for), and
    expect["host"]    the values the executor evaluates on the host -- Shape and the arithmetic on it -- whose cached device copies the sessions rely on.
No case feeds a host-evaluated value into a device Gather / Scatter index: a stale shape constant can then change values, never an address.

A session is a list of actions, `(words of the script line, binding whose values the action's outputs must carry or None)`; `write_session` puts the
model, the bindings and the script into a directory and `read_script` reads a script back.  The cases are NOT part of graph_fuzz.ROWS / corpus()."""
import functools
import os
import subprocess

import numpy as np

from tests import graph_fuzz as gf
from rten_amd import onnx_writer as ow

F = np.float32
SESSIONS = ("walk", "capture_survives", "recapture", "plans_elsewhere", "outputs_outlive")
OUTLIVE_CASES = ("shape_scalars", "conv_reshape_matmul")  # the cases whose outputs include views and host-evaluated values
# `plans_elsewhere` tunes first, and a step autotune left a plan on takes no shape-keyed entry; this session gives the table to an untuned graph, so that the
# entries are taken at the first binding and then STAY on the steps at other shapes (Graph::run: "the entry stays").  For the cases with MatMul-family steps.
PLANNED_SESSION, PLANNED_CASES = "shape_plans_stay", ("conv_reshape_matmul", "attention")
# non-default launch plans [variant, split mode, K groups, tile order] for the shape-keyed table of `plans_elsewhere`: the entries
# tests/test_shape_arithmetic.py gives the model ABI (all bit-exact by contract: exact split-K, tile shape and order change no sum's order)
SHAPE_PLANS = ([1, 3, 1, 0], [3, 3, 1, 1], [2, 3, 1, 0], [3, 1, 2, 0])


def _values(seed):
    return gf.Builder("binding", seed)


def _finish(b, more, steps, host):
    """`more`: the bindings after the first, the last of them repeating the first one's shapes."""
    b.alt = more[0]
    c = b.finish()
    c.bindings += more[1:]
    first, last = c.bindings[0], c.bindings[-1]
    assert all(first[k].shape == last[k].shape for k in first) and any(not np.array_equal(first[k], last[k]) for k in first), c.name
    c.expect["steps"] = list(steps)
    c.expect["host"] = list(host)
    return c


def _dim(b, shp, axis):
    """Shape -> Gather(scalar index) -> Unsqueeze: one dimension as a [1] vector, as exporters write it."""
    return b.node("Unsqueeze", [b.node("Gather", [shp, b.const(np.array(axis, np.int64), "i")], axis=0), b.ci([0])])


def conv_reshape_matmul():
    """graph_fuzz.shape_case with the batch bound at 1 .. 10: Conv + Relu, flattened through Shape -> Gather -> Unsqueeze -> Concat -> Reshape, MatMul + bias."""
    b = gf.Builder("session_conv_reshape_matmul", seed=3101)
    x = b.inp((1, 3, 6, 6), dims=["batch", 3, 6, 6])
    y = b.node("Relu", [b.node("Conv", [x, b.cf((4, 3, 3, 3), 0.4), b.cf((4,))], kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[1, 1])])
    shp = b.node("Shape", [y])
    tgt = b.node("Concat", [_dim(b, shp, 0), b.ci([-1])], axis=0)
    flat = b.node("Reshape", [y, tgt])
    z = b.node("Add", [b.node("MatMul", [flat, b.cf((4 * 36, 10), 0.2)]), b.cf((10,))])
    b.out(z)
    b.out(flat)
    b.row("session/conv_reshape_matmul", 2, ["Conv+Relu", "FusedMatMul"])
    b.case.expect["modes_differ"] = "FusedMatMul bias position"
    v = _values(3111)
    return _finish(b, [{x: v.data((n, 3, 6, 6))} for n in list(range(2, 11)) + [1]], ["Conv+Relu", "FusedMatMul", "Reshape(view)"], [shp, tgt])


ATTENTION_SHAPES = [(1, 1), (2, 2), (3, 7), (1, 16), (2, 17), (3, 33), (3, 64), (2, 100), (1, 128), (1, 129), (1, 130)]  # (batch, seq): 129, 130 are past the fused kernel's key limit


def _attention_binding(v, batch, seq):
    mask = (v.rng.random((batch, seq)) < 0.7).astype(np.int64)
    mask[:, 0] = 1  # no row without a key: a fully masked row is a uniform softmax in f32 by absorption only
    return v.data((batch, seq, 128)), mask


def attention():
    """One self-attention block as an exporter writes it with dynamic axes: two heads of 64 split and merged through Shape -> Gather -> Unsqueeze -> Concat ->
    Reshape, a 0 / 1 mask through Equal / Where / Expand with the target Where(Equal(shape, -1), ones, shape), then the output projection, Add and
    LayerNormalization.  Plans as FusedMatMul(QKV), MultiHeadSdpa over its column blocks, FusedMatMul and Add+LayerNormalization."""
    b = gf.Builder("session_attention", seed=3102)
    (B0, S0), v = ATTENTION_SHAPES[0], _values(3112)
    x0, m0 = _attention_binding(v, B0, S0)
    x = b.inp(None, dims=["batch", "seq", 128], arr=x0)
    mask = b.inp(None, dims=["batch", "seq"], arr=m0)
    q, k, vv = (b.node("Add", [b.node("MatMul", [x, b.cf((128, 128), 0.15)]), b.cf((128,), 0.2)]) for _ in range(3))
    shp = b.node("Shape", [x])
    bdim, sdim = _dim(b, shp, 0), _dim(b, shp, 1)
    splits = []  # one target per Reshape, as exporters write them (the attention pre-pass reads a run-time target only from a Concat of its own)

    def heads(t, perm):
        splits.append(b.node("Concat", [bdim, sdim, b.ci([2]), b.ci([64])], axis=0))
        return b.node("Transpose", [b.node("Reshape", [t, splits[-1]])], perm=perm)
    cond = b.node("Equal", [b.node("Unsqueeze", [mask, b.ci([1, 2])]), b.const(np.array(1, np.int64), "i")])
    addend = b.node("Where", [cond, b.const(np.array(0.0, F)), b.const(np.array(-3.4e38, F))])
    raw = b.node("Concat", [bdim, b.ci([1]), sdim, b.ci([-1])], axis=0)
    tgt = b.node("Where", [b.node("Equal", [raw, b.ci([-1])]), b.ci([1, 1, 1, 1]), raw])
    expanded = b.node("Expand", [addend, tgt])  # (before the scores: the attention pre-pass takes a mask only if it exists when its step runs)
    scores = b.node("Div", [b.node("MatMul", [heads(q, [0, 2, 1, 3]), heads(k, [0, 2, 3, 1])]), b.const(np.array(8.0, F))])
    probs = b.node("Softmax", [b.node("Add", [scores, expanded])], axis=-1)
    merged = b.node("Transpose", [b.node("MatMul", [probs, heads(vv, [0, 2, 1, 3])])], perm=[0, 2, 1, 3])
    merge = b.node("Concat", [bdim, sdim, b.ci([128])], axis=0)
    attn = b.node("Reshape", [merged, merge])
    proj = b.node("Add", [b.node("MatMul", [attn, b.cf((128, 128), 0.15)]), b.cf((128,), 0.2)])
    y = b.node("LayerNormalization", [b.node("Add", [proj, x]), b.cf((128,)), b.cf((128,))], axis=-1, epsilon=1e-5)
    b.out(y)
    b.row("session/attention")
    b.case.expect["modes_differ"] = "FusedMatMul bias position"
    more = [dict(zip((x, mask), _attention_binding(v, bt, s))) for bt, s in ATTENTION_SHAPES[1:] + [ATTENTION_SHAPES[0]]]
    return _finish(b, more, ["FusedMatMul(QKV)", "MultiHeadSdpa(QKV column blocks)", "FusedMatMul", "Add+LayerNormalization"], [shp] + splits + [merge, tgt])


INT8_SHAPES = [(1, 3, 3), (2, 4, 5), (3, 5, 4), (1, 6, 6), (2, 7, 9), (3, 8, 8), (1, 9, 12), (2, 10, 3), (3, 11, 7), (1, 12, 12)]  # (batch, H, W)


def int8_chain():
    """DynamicQuantizeLinear -> ConvInteger 3x3 (unpadded) -> Cast -> Mul -> Add -> Relu -> DynamicQuantizeLinear -> ConvInteger 1x1 -> Cast -> Mul with batch, H
    and W dynamic: two staged quantizers, the second on the statistics its producer's launch leaves in the graph's arena, and two ConvIntegerToFloat steps."""
    b = gf.Builder("session_int8_chain", seed=3103)
    r = b.rng
    C, O, O2 = 4, 4, 6
    n0, h0, w0 = INT8_SHAPES[0]
    x = b.inp((n0, C, h0, w0), dims=["batch", C, "height", "width"])
    zero = b.const(np.zeros((), np.int8))

    def conv(src, k, cout, cin):
        qx, xs, xz = b.node("DynamicQuantizeLinear", [src], nout=3)
        wq = b.const(r.integers(-64, 65, (cout, cin, k, k)).astype(np.int8))
        acc = b.node("ConvInteger", [qx, wq, xz, zero], kernel_shape=[k, k], pads=[0, 0, 0, 0], strides=[1, 1])
        return b.node("Mul", [b.node("Cast", [acc], to=ow.FLOAT), b.node("Mul", [xs, b.const(np.array(0.0123, F))])])
    hidden = b.node("Relu", [b.node("Add", [conv(x, 3, O, C), b.cf((1, O, 1, 1))])])
    y = conv(hidden, 1, O2, O)
    b.out(y)
    b.row("session/int8_chain")
    v = _values(3113)
    more = [{x: v.data((n, C, h, w))} for n, h, w in INT8_SHAPES[1:] + [INT8_SHAPES[0]]]
    steps = ["DynamicQuantizeLinear(staged)", "ConvIntegerToFloat+bias+Relu", "DynamicQuantizeLinear(staged, producer statistics)", "ConvIntegerToFloat"]
    return _finish(b, more, steps, [])


SCALAR_LENGTHS = [1, 15, 16, 17, 257, 2, 5, 33, 64, 100]


def shape_scalars():
    """Values the host computes from a dynamic last axis used as DATA: the mean as ReduceSum(x, -1) / Cast(len) (Div by a one-element divisor the host knows:
    the uploaded reciprocal), x * Cast(len), and graph outputs that ARE host-evaluated values -- Shape(x), Concat(Shape(x)[0:1], [-1]) and Cast(len)."""
    b = gf.Builder("session_shape_scalars", seed=3104)
    x = b.inp((3, SCALAR_LENGTHS[0]), dims=[3, "len"])
    shp = b.node("Shape", [x])
    flen = b.node("Cast", [b.node("Gather", [shp, b.const(np.array(-1, np.int64), "i")], axis=0)], to=ow.FLOAT)
    mean = b.node("Div", [b.node("ReduceSum", [x, b.ci([-1])], keepdims=1), flen])
    scaled = b.node("Mul", [x, flen])
    rows = b.node("Concat", [b.node("Slice", [shp, b.ci([0]), b.ci([1])]), b.ci([-1])], axis=0)
    for o in (mean, shp, rows, flen, scaled):
        b.out(o)
    b.row("session/shape_scalars")
    v = _values(3114)
    return _finish(b, [{x: v.data((3, n))} for n in SCALAR_LENGTHS[1:] + [SCALAR_LENGTHS[0]]], ["Shape", "ReduceSum", "Div", "Mul"], [shp, flen])


RNN_SHAPES = [(1, 1), (2, 2), (3, 3), (4, 1), (5, 2), (6, 3), (7, 1), (8, 2), (9, 3), (5, 1)]  # (seq, batch): both sides of the 5-step weight prepacking, one row and more


def rnn_dynamic():
    """A bidirectional GRU (hidden 8, input 5) and an LSTM behind it, sequence length and batch dynamic; the directions are merged through a Reshape whose target
    is computed from Shape(x)."""
    b = gf.Builder("session_rnn_dynamic", seed=3105)
    s0, n0 = RNN_SHAPES[0]
    x = b.inp((s0, n0, 5), dims=["seq", "batch", 5])
    gy, gh = b.node("GRU", [x, b.cf((2, 24, 5), 0.5), b.cf((2, 24, 8), 0.5), b.cf((2, 48), 0.3)], nout=2, hidden_size=8, direction="bidirectional", linear_before_reset=1)
    shp = b.node("Shape", [x])
    tgt = b.node("Concat", [b.node("Slice", [shp, b.ci([0]), b.ci([2])]), b.ci([16])], axis=0)
    both = b.node("Reshape", [b.node("Transpose", [gy], perm=[0, 2, 1, 3]), tgt])
    ly, lh = b.node("LSTM", [both, b.cf((1, 24, 16), 0.4), b.cf((1, 24, 6), 0.4), b.cf((1, 48), 0.3)], nout=2, hidden_size=6, direction="forward")
    for o in (ly, lh, gh):
        b.out(o)
    b.row("session/rnn_dynamic")
    v = _values(3115)
    return _finish(b, [{x: v.data((s, n, 5))} for s, n in RNN_SHAPES[1:] + [RNN_SHAPES[0]]], ["GRU", "LSTM"], [shp, tgt])


CASES = {"conv_reshape_matmul": conv_reshape_matmul, "attention": attention, "int8_chain": int8_chain, "shape_scalars": shape_scalars, "rnn_dynamic": rnn_dynamic}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name, binding):
    """The interpreter's values of one binding, computed once and shared (read-only) by every session and test."""
    vals = gf.evaluate(case(name), binding, fused=True)
    for a in vals.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return vals


def gemm_shapes(name):
    """["gemm:MxKxN"] of the first binding's MatMul-family steps, as Graph::run spells the keys of a shape-keyed plan table: M = the rows of A over all
    its leading dims, for every MatMul / Gemm whose right operand is a 2-D constant -- and the merged QKV projection of an attention block (N = 3 x hidden)."""
    c, vals = case(name), expected(name, 0)
    keys, by_lhs = [], {}
    for n in c.nodes:
        if n["op"] in ("MatMul", "Gemm") and n["inputs"][1] in c.inits and c.inits[n["inputs"][1]].ndim == 2:
            a, w = vals[n["inputs"][0]], c.inits[n["inputs"][1]]
            kdim, ncols = (w.shape[1], w.shape[0]) if n["attrs"].get("transB", 0) else w.shape
            keys.append(f"gemm:{a.size // a.shape[-1]}x{kdim}x{ncols}")
            by_lhs.setdefault(n["inputs"][0], []).append((a.size // a.shape[-1], kdim, ncols))
    for group in by_lhs.values():
        if len(group) == 3 and len(set(group)) == 1:
            keys.append("gemm:%dx%dx%d" % (group[0][0], group[0][1], 3 * group[0][2]))
    return sorted(set(keys))


# ------------------------------------------------------------------------------------------------ sessions
def walk_order(n, seed=20240):
    """Every binding in ascending, descending and seeded-shuffled order, then the first again."""
    return list(range(n)) + list(range(n - 1, -1, -1)) + [int(k) for k in np.random.default_rng(seed).permutation(n)] + [0]


def session(name, kind):
    """[(words, binding or None)]: a word is text, ("in", k) for binding k's input file, "@" for an output file (write_session numbers them) or "shape_plans"
    for the case's shape-keyed plan table.  The binding is the one whose values the action's outputs must carry."""
    n = len(case(name).bindings)
    last = n - 1  # the first shape again, other values
    run = lambda k: (["run", ("in", k), "@"], k)
    capture = lambda k: (["capture", ("in", k), "@"], k)
    if kind == "walk":
        return [run(k) for k in walk_order(n)]
    if kind == "capture_survives":
        return ([capture(0), (["replay", "@"], 0)] + [run(k) for k in range(1, last)] +
                [(["replay", "@"], 0), (["refill", ("in", last)], None), (["replay", "@"], last)])
    if kind == "recapture":
        return [capture(0), (["replay", "@"], 0), capture(5), (["replay", "@"], 5), capture(0), (["replay", "@"], 0)]
    if kind == "plans_elsewhere":
        return [(["tune", ("in", 0)], None)] + [run(k) for k in walk_order(n)] + [(["shape-plans", "shape_plans"], None), run(1), run(0), run(1)]
    if kind == PLANNED_SESSION:  # no match, the entries taken, the same steps at other shapes; a re-plan (entries go with their table), taken again
        plans = (["shape-plans", "shape_plans"], None)
        return [plans, run(1), run(0), run(1), run(last - 1), run(0), plans, run(1), run(0)]
    if kind == "outputs_outlive":
        return ([(["hold", ("in", 0), "a"], None), (["hold", ("in", 0), "b"], None), (["distinct", "a", "b"], None)] + [run(k) for k in range(1, n)] +
                [(["read", "a", "@"], 0), (["read", "b", "@"], 0)])
    raise KeyError(kind)


def format_script(actions):
    return "".join(" ".join(words) + "\n" for words in actions)


def read_script(text):
    return [line.split("#", 1)[0].split() for line in text.splitlines() if line.split("#", 1)[0].split()]


def write_session(name, kind, directory):
    """Writes model.onnx, b<k>.safetensors, shape_plans.txt and script.txt into `directory`.  Returns (model path, script path, [(line number, output path,
    binding)] for the actions that write outputs)."""
    from safetensors.numpy import save_file
    c = case(name)
    path = lambda f: os.path.join(directory, f)
    with open(path("model.onnx"), "wb") as f:
        f.write(c.onnx)
    for k, binding in enumerate(c.bindings):
        save_file({nm: np.ascontiguousarray(a) for nm, a in binding.items()}, path(f"b{k}.safetensors"))
    with open(path("shape_plans.txt"), "w") as f:
        for i, key in enumerate(gemm_shapes(name)):
            f.write(key + " " + " ".join(str(v) for v in SHAPE_PLANS[i % len(SHAPE_PLANS)]) + "\n")
    actions, outputs = [], []
    for line, (words, binding) in enumerate(session(name, kind), start=1):
        real = []
        for w in words:
            if w == "@":
                outputs.append((line, path(f"out{line}.safetensors"), binding))
                real.append(outputs[-1][1])
            elif w == "shape_plans":
                real.append(path("shape_plans.txt"))
            elif isinstance(w, tuple):
                real.append(path(f"b{w[1]}.safetensors"))
            else:
                real.append(w)
        actions.append(real)
    with open(path("script.txt"), "w") as f:
        f.write(format_script(actions))
    return path("model.onnx"), path("script.txt"), outputs


# ------------------------------------------------------------------------------------------------ the probe
PROBE = os.path.join(gf.ROOT, "tests", "cpp", "_build", "graph_session")
PROBE_SRC = os.path.join(gf.ROOT, "tests", "cpp", "graph_session.cpp")


def build_session_probe(sanitize=False):
    """tests/cpp/graph_session.cpp, built on demand like graph_fuzz.build_outlive_probe.  sanitize=True: a second binary under AddressSanitizer and
    UndefinedBehaviorSanitizer for the probe's host-only half (`--check-script`: the script parser, the plan tables, Safetensors I/O); it never opens a device."""
    from rten_amd import lib as L
    L.load()
    out = PROBE + ("_asan" if sanitize else "")
    deps = [PROBE_SRC] + [os.path.join(gf.ROOT, "include", h) for h in ("rten_hip_graph.hpp", "rten_hip_ops.hpp", "rten_hip_safetensors.hpp", "rten_hip.h")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        # (the sanitizer runtimes linked statically: the program then runs whatever else the environment loads into a process first)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
        subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I" + os.path.join(gf.ROOT, "include"), PROBE_SRC, "-o", out,
                               "-L" + os.path.join(gf.ROOT, "rten_amd"), "-lrten_hip", "-Wl,-rpath,$ORIGIN/../../../rten_amd",
                               "-Wl,-rpath," + os.path.join(gf.ROOT, "rten_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return out
