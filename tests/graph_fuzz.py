"""Seeded generator of small adversarial ONNX graphs for the graph executor (include/rten_hip_graph.hpp), and a node-by-node interpreter of them.

A graph is assembled from MOTIFS -- one fusable pattern of Graph::compile each, optionally carrying one SPOILER that must disable or reroute the
fusion -- joined by inert glue.  `ROWS` is the table of (motif, variant) pairs; every row has one hand-written minimal graph (`hand_case`) and occurs
again inside the random graphs of `make_case(seed)`.  Each motif records in `Case.expect` what the executor's plan must look like: how many nodes the
fusion passes fold away (`folded`) and the kinds of the fused steps (`kinds`).

`evaluate(case, binding, fused)` walks the node list once and evaluates every node by itself on the CPU oracle (oracle/ref.py, oracle/einsum.py), the
numpy restatements in tests/ (select_rules.py, test_gpu_activations.np_act) or plain numpy (single IEEE operations and layout ops are exact): no buffer
reuse, no views, no reordering.  Its semantics are the reference's.  The executor's own fusions are bit-identical to the operators they replace, so
they need no rule here; the reference's optimiser changes arithmetic in two places, and the interpreter applies those rules exactly where the
reference's pattern matches (`_reference_matmul_fusions`):
  * MatMulAddFusion  (src/optimize/fusions.rs:806-847): Add(MatMul(a, b), bias) with a constant rank-1 bias -> FusedMatMul(a, b, bias); the GEMM adds
    the bias after the FIRST depth block of 256 (rten-gemm/src/lib.rs:876-891), not after the last, so K > 256 rounds differently;
  * MatMulScaleFusion (src/optimize/fusions.rs:855-960): Mul(MatMul, c), Mul(c, MatMul) or Div(MatMul, c) with a constant scalar c -> FusedMatMul with
    alpha = c or 1 / c; alpha is applied per depth block and a division becomes a multiplication by the rounded reciprocal.
With fused=False (the executor's --no-fuse mode) every node is evaluated as the graph spells it; cases where the two differ are exactly the MatMul
motif's (`Case.expect["modes_differ"]` says so).
In BOTH modes the interpreter first rewrites the graph as the loader's canonicalisation must (`canonical`): the reference's Silu / Swish / Gelu /
LayerNormalization idiom fusions, `Constant` nodes and constant DequantizeLinear folding, by the rules restated in tests/fusion_rules.py -- Graph::compile
canonicalises whether or not its own fusions are on.  `Case.expect["canonical"]` is the operator count of that form (None where nothing is rewritten).

The first table (OLD_ROWS) and the seeds below OLD_SEEDS are frozen (tests/golden/graph_fuzz_corpus.json holds their hashes); the rows added later (idiom/*,
attention/*, norm_act/*, qdq/*) and the glue of the later operator families (`glue_later`) are drawn by the seeds from OLD_SEEDS on only.
  * A fused bias whose length is not N: the reference's FusedMatMul reaches gemm's WrongBiasSize ("bias vector length is incorrect",
    rten-gemm/src/lib.rs:809-816) through an unwrap (src/ops/matmul.rs:361-374), i.e. it does not run the graph; the executor reports
    IncompatibleInputShapes "Cannot broadcast bias to output shape".  Pinned as an expected error of the fused modes.

`evaluate64` is an independent float64 evaluation (numpy / torch-CPU only, nothing shared with oracle/) used by tests/test_graph_fuzz_oracle.py.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rten_amd import onnx_writer as ow  # noqa: E402

F = np.float32
N_SEEDS = 96          # the committed random corpus: make_case(0) .. make_case(N_SEEDS - 1)
OLD_SEEDS = 64        # seeds below this walk the first table (OLD_ROWS) and stay byte-identical (tests/golden/graph_fuzz_corpus.json); the others walk NEW_ROWS
MAX_NODES_NEW = 72    # a seed of the extended table forces two or three idiom rows of up to 16 nodes each
MAX_ELEMS = 1 << 16   # no tensor of a generated graph is larger

ACT_KINDS = ("Sigmoid", "Silu", "Swish", "HardSigmoid", "HardSwish", "LeakyRelu", "Elu", "Clip")
# kinds of fused steps as Graph::compile names them; plain operators are not listed in Case.expect["kinds"]
FUSED_PREFIXES = ("FusedMatMul", "AddSoftmax", "ConvIntegerToFloat", "MatMulIntegerToFloat", "MultiHeadSdpa")


def is_fused_kind(kind):
    return "+" in kind or kind.startswith(FUSED_PREFIXES)


class Case:
    def __init__(self, name):
        self.name = name
        self.nodes = []          # dicts: op, inputs, outputs, attrs, name
        self.inits = {}          # name -> ndarray (insertion order = file order)
        self.input_specs = []    # (name, declared dims)
        self.bindings = [{}]     # one dict of named numpy inputs per run; more than one when a dynamic axis is bound at several sizes
        self.outputs = []        # ordered graph output names (a name may occur twice)
        self.expect = {"rows": [], "folded": 0, "kinds": [], "error": None, "modes_differ": None, "canonical": None, "canonical_nodes": None, "off_nominal": None, "folded_dequantize": None}
        self.onnx = b""

    @property
    def inputs(self):
        return self.bindings[0]


# ------------------------------------------------------------------------------------------------ node-by-node evaluation (f32, the oracle)
def _act32(op, x, attrs, consts):
    from rten_amd import lib as L
    from tests.test_gpu_activations import np_act, FMAX
    if op == "Relu":
        return np_act(L.ACT_RELU, x)
    if op == "Gelu":
        return np_act(L.ACT_GELU, x)
    if op == "Sigmoid":
        return np_act(L.ACT_SIGMOID, x)
    if op == "Silu":
        return np_act(L.ACT_SILU, x)
    if op == "Swish":
        return np_act(L.ACT_SWISH, x, attrs.get("alpha", 1.0))
    if op == "HardSigmoid":
        return np_act(L.ACT_HARD_SIGMOID, x, attrs.get("alpha", 0.2), attrs.get("beta", 0.5))
    if op == "HardSwish":
        return np_act(L.ACT_HARD_SWISH, x)
    if op == "LeakyRelu":
        return np_act(L.ACT_LEAKY_RELU, x, attrs.get("alpha", 0.01))
    if op == "Elu":
        return np_act(L.ACT_ELU, x, attrs.get("alpha", 1.0))
    if op == "Clip":
        lo = consts[0] if consts and consts[0] is not None else -FMAX
        hi = consts[1] if len(consts) > 1 and consts[1] is not None else FMAX
        return np_act(L.ACT_CLIP, x, float(lo), float(hi))
    raise KeyError(op)


def _conv_geometry(x, w, attrs):
    """(x4, w4, pads4, strides2, dilations2, one_d) of a 1-D or 2-D Conv / ConvInteger node."""
    one_d = x.ndim == 3
    nsp = 1 if one_d else 2
    pads = list(attrs.get("pads", [0] * (2 * nsp)))
    strides = list(attrs.get("strides", [1] * nsp))
    dil = list(attrs.get("dilations", [1] * nsp))
    if one_d:  # src/ops/conv.rs:142-182: a 1-D convolution is the 2-D one on [N, C, 1, L]
        return x[:, :, None, :], w[:, :, None, :], (0, pads[0], 0, pads[1]), (1, strides[0]), (1, dil[0]), True
    return x, w, tuple(pads), tuple(strides), tuple(dil), False


def _slice_np(x, starts, ends, axes, steps):
    sl = [slice(None)] * x.ndim
    for s, e, a, st in zip(starts, ends, axes, steps):
        sl[int(a)] = slice(int(s), int(e), int(st))
    return np.ascontiguousarray(x[tuple(sl)])


def _layout_op(op, ins, attrs):
    """Operators that only move or index data, shared by both evaluators' callers through plain numpy (exact in any precision)."""
    x = ins[0]
    if op == "Identity":
        return [x.copy()]
    if op == "Reshape":
        shape = [x.shape[i] if d == 0 else int(d) for i, d in enumerate(np.asarray(ins[1]).ravel())]
        return [x.reshape(shape)]
    if op == "Flatten":
        a = attrs.get("axis", 1)
        a = a + x.ndim if a < 0 else a
        return [x.reshape(int(np.prod(x.shape[:a], dtype=np.int64)), -1)]
    if op == "Squeeze":
        return [np.squeeze(x, tuple(int(a) for a in np.asarray(ins[1]).ravel()))]
    if op == "Unsqueeze":
        y = x
        nd = x.ndim + np.asarray(ins[1]).size
        for a in sorted(int(a) % nd for a in np.asarray(ins[1]).ravel()):
            y = np.expand_dims(y, a)
        return [y]
    if op == "Transpose":
        return [np.ascontiguousarray(np.transpose(x, attrs.get("perm")))]
    if op == "Concat":
        return [np.concatenate(ins, axis=attrs["axis"])]
    if op == "Slice":
        n = len(ins[1])
        axes = ins[3] if len(ins) > 3 and ins[3] is not None else np.arange(n)
        steps = ins[4] if len(ins) > 4 and ins[4] is not None else np.ones(n, np.int64)
        return [_slice_np(x, ins[1], ins[2], axes, steps)]
    if op == "Split":
        cuts = np.cumsum(np.asarray(ins[1]).ravel())[:-1]
        return [np.ascontiguousarray(p) for p in np.split(x, cuts, axis=attrs.get("axis", 0))]
    if op == "Shape":
        return [np.array(x.shape, np.int64)]
    if op == "Gather":
        return [np.take(x, np.asarray(ins[1]), axis=attrs.get("axis", 0))]
    return None


LAYOUT_OPS = ("Identity", "Reshape", "Flatten", "Squeeze", "Unsqueeze", "Transpose", "Concat", "Slice", "Split", "Shape", "Gather")


GLUE_OPS = ("Equal", "Where", "Expand", "ConstantOfShape")
_CAST_TO = {ow.FLOAT: np.float32, ow.INT32: np.int32, ow.INT64: np.int32, ow.UINT8: np.uint8, ow.INT8: np.int8}


def _narrow(a):
    """int64 is int32 from load on (onnx_loader.rs:332-339, saturating): what every integer value of a graph is to the executor."""
    a = np.asarray(a)
    return np.clip(a, -(1 << 31), (1 << 31) - 1).astype(np.int32) if a.dtype == np.int64 else a


def _resize_nearest_x2(x, ins, attrs):
    """Resize as the glue writes it: mode nearest, scales [1, 1, 2, 2], default half_pixel / round_prefer_floor.  Output o reads input round_prefer_floor((o + 0.5) / 2
    - 0.5) = o // 2 (-0.25 -> 0, 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, ...): every element repeated twice along both axes -- data movement, exact in any precision."""
    assert attrs.get("mode") == "nearest" and [float(v) for v in ins[2]] == [1.0, 1.0, 2.0, 2.0] and x.ndim == 4, (attrs, ins[2])
    return np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)


def reference_div(a, b):
    """Div as the reference computes it (binary_elementwise.rs:613-637): a float divisor of exactly one element, at any rank, multiplies by its reciprocal,
    a * (1 / b), each step rounded in the operands' type; every other divisor divides (tests/glue_rules.py states the rule with its evidence)."""
    a, b = np.asarray(a), np.asarray(b)
    if b.size == 1 and b.dtype.kind == "f":
        return a * (b.dtype.type(1) / b)
    return np.divide(a, b)


def eval_node(node, ins):
    """One node on the f32 oracle.  `ins`: the input arrays (None for an omitted optional input).  Returns the list of outputs."""
    from oracle import einsum as OE
    from oracle import ref
    from tests import glue_rules as GR
    from tests import index_rules as IR
    from tests import math_rules as MR
    from tests import reduce_rules as RDR
    from tests import sample_rules as SMR
    from tests import norm_rules as NR
    from tests import qdq_rules as QR
    from tests import rnn_rules as RR
    from tests import select_rules as SR
    op, attrs = node["op"], node["attrs"]
    if op in LAYOUT_OPS:
        return _layout_op(op, ins, attrs)
    x = ins[0] if ins else None
    with np.errstate(all="ignore"):
        if op in ("Add", "Sub", "Mul", "Div"):  # one correctly rounded IEEE operation per element: numpy is exact
            fn = {"Add": np.add, "Sub": np.subtract, "Mul": np.multiply, "Div": reference_div}[op]  # (Div: two operations for a one-element divisor)
            return [np.asarray(fn(ins[0], ins[1]), ins[0].dtype)]
        if op == "Conv":
            x4, w4, pads, strides, dil, one_d = _conv_geometry(x, ins[1], attrs)
            y = ref.conv2d_f32(x4, w4, ins[2] if len(ins) > 2 else None, pads=pads, strides=strides, dilations=dil, groups=attrs.get("group", 1))
            return [y[:, :, 0, :] if one_d else y]
        if op == "ConvInteger":
            x4, w4, pads, strides, dil, _ = _conv_geometry(x, ins[1], attrs)
            assert not any(pads), "the corpus keeps int8 convolutions unpadded"
            wzp = ins[3] if len(ins) > 3 and ins[3] is not None else None
            return [ref.conv2d_int8(x4, w4, x_zp=int(ins[2]), w_zp=wzp, pads=pads, strides=strides, dilations=dil, groups=attrs.get("group", 1))]
        if op == "Cast":
            if attrs["to"] == ow.FLOAT and x.dtype != np.int64:
                return [x.astype(F)]
            return [GR.cast(_narrow(x), _CAST_TO[attrs["to"]])]
        if op in GLUE_OPS:  # the shape-polymorphic graphs of tests/graph_sessions.py: the reference's rules as tests/glue_rules.py states them
            ins = [None if a is None else _narrow(a) for a in ins]
            if op == "Equal":
                return [GR.compare("Equal", ins[0], ins[1])]
            if op == "Where":
                return [GR.where(ins[0], ins[1], ins[2])]
            if op == "Expand":
                return [GR.expand(ins[0], ins[1])]
            fill = attrs.get("value")
            return [GR.constant_of_shape(ins[0], None if fill is None else np.asarray(fill).reshape(-1)[0])]
        if op in ("GRU", "LSTM"):  # tests/rnn_rules.py; outputs Y, Y_h (, Y_c)
            kw = dict(b=ins[3] if len(ins) > 3 else None, direction=attrs.get("direction", "forward"))
            assert all(a is None for a in ins[4:]), "the session graphs give no sequence_lens / initial state"
            return list((RR.gru if op == "GRU" else RR.lstm)(ins[0], ins[1], ins[2], **kw))
        if op == "DynamicQuantizeLinear":
            q, s, z = ref.dynamic_quantize_linear(x)
            return [q, np.asarray(s, F), np.asarray(z, np.uint8)]
        if op == "MatMul":
            return [ref.matmul_f32(ins[0], ins[1])]
        if op == "FusedMatMul":  # only ever made by _reference_matmul_fusions
            return [ref.matmul_f32(ins[0], ins[1], alpha=attrs.get("alpha", 1.0), bias=ins[2] if len(ins) > 2 else None)]
        if op == "Gemm":
            a = ins[0].T if attrs.get("transA", 0) else ins[0]
            b = ins[1].T if attrs.get("transB", 0) else ins[1]
            if len(ins) > 2 and ins[2] is not None:
                c = np.broadcast_to(ins[2], (a.shape[0], b.shape[1])).astype(F)
                return [ref.gemm_f32(a, b, c=c, alpha=attrs.get("alpha", 1.0), beta=attrs.get("beta", 1.0))]
            return [ref.gemm_f32(a, b, alpha=attrs.get("alpha", 1.0), beta=0.0)]
        if op == "LayerNormalization":
            a = attrs.get("axis", -1)
            a = a + x.ndim if a < 0 else a
            cols = int(np.prod(x.shape[a:], dtype=np.int64))
            bias = ins[2].reshape(-1) if len(ins) > 2 and ins[2] is not None else None
            return [ref.layer_norm(x.reshape(-1, cols), ins[1].reshape(-1), bias, eps=attrs.get("epsilon", 1e-5)).reshape(x.shape)]
        if op == "Softmax":
            a = attrs.get("axis", -1)
            return [np.ascontiguousarray(np.moveaxis(ref.softmax(np.ascontiguousarray(np.moveaxis(x, a, -1))), -1, a))]
        if op == "MaxPool":
            return [ref.max_pool(x, attrs["kernel_shape"], attrs.get("strides", [1, 1]), attrs.get("pads", [0, 0, 0, 0]))]
        if op == "AveragePool":
            return [ref.average_pool(x, attrs["kernel_shape"], attrs.get("strides", [1, 1]), attrs.get("pads", [0, 0, 0, 0]))]
        if op == "GlobalAveragePool":
            return [ref.global_average_pool(x)]
        if op == "ReduceSum":
            return [OE.reduce_sum(x, [int(a) for a in ins[1]], bool(attrs.get("keepdims", 1)))]
        if op == "ReduceMean":  # axes: the attribute, or from opset 18 on a constant input
            axes = list(attrs["axes"]) if "axes" in attrs else [int(a) for a in ins[1]]
            return [OE.reduce_mean(x, axes, bool(attrs.get("keepdims", 1)))]
        if op == "Tanh":
            return [ref.tanh(x)]
        if op == "Constant":
            return [np.asarray(attrs["value"])]
        if op == "Erf":
            return [ref.erf(x)]
        if op in MR.UNARY:
            return [MR.UNARY[op](x)]
        if op == "Pow":
            return [MR.pow_(x, ins[1])]
        if op == "Pad":
            return [MR.pad(x, ins[1], mode=attrs.get("mode", "constant"), value=F(0) if len(ins) < 3 or ins[2] is None else F(np.asarray(ins[2]).reshape(-1)[0]))]
        if op in ("Max", "Mean"):
            return [(MR.vmax if op == "Max" else MR.mean)(*ins)]
        if op in ("ReduceL2", "ReduceLogSumExp"):
            return [RDR.reduce({"ReduceL2": "l2", "ReduceLogSumExp": "log_sum_exp"}[op], x, [int(a) for a in ins[1]], bool(attrs.get("keepdims", 1)))]
        if op == "ReduceMax":
            return [SR.reduce_minmax(x, [int(a) for a in ins[1]], bool(attrs.get("keepdims", 1)), "max")]
        if op == "GlobalMaxPool":
            return [RDR.global_max_pool(x)]
        if op == "CumSum":
            return [IR.cum_sum(x, int(np.asarray(ins[1]).reshape(-1)[0]), bool(attrs.get("exclusive", 0)), bool(attrs.get("reverse", 0)))]
        if op == "Trilu":
            return [IR.trilu(x, int(np.asarray(ins[1]).reshape(-1)[0]) if len(ins) > 1 and ins[1] is not None else 0, bool(attrs.get("upper", 1)))]
        if op == "Tile":
            return [IR.tile(x, [int(r) for r in ins[1]])]
        if op == "GatherElements":
            return [IR.gather_elements(x, np.asarray(ins[1]), attrs.get("axis", 0))]
        if op == "DepthToSpace":
            return [SMR.depth_to_space(x, attrs["blocksize"], attrs.get("mode", "DCR"))]
        if op == "Resize":
            return [_resize_nearest_x2(x, ins, attrs)]
        if op == "InstanceNormalization":
            return [NR.instance_norm(x, ins[1], ins[2], eps=attrs.get("epsilon", 1e-5))]
        if op == "BatchNormalization":
            return [NR.batch_norm(x, ins[1], ins[2], ins[3], ins[4], eps=attrs.get("epsilon", 1e-5))]
        if op == "LogSoftmax":
            return [NR.log_softmax(x, axis=attrs.get("axis", -1))]
        if op == "QuantizeLinear":
            return [QR.quantize_linear(x, ins[1], ins[2] if len(ins) > 2 else None, axis=attrs.get("axis", -1))]
        if op == "DequantizeLinear":
            return [QR.dequantize_linear(x, ins[1], ins[2] if len(ins) > 2 else None, axis=attrs.get("axis", 1))]
        if op == "ArgMax":
            return [SR.arg_minmax(x, attrs.get("axis", 0), bool(attrs.get("keepdims", 1)), "max")]
        if op == "TopK":
            v, i = SR.topk(x, int(np.asarray(ins[1]).ravel()[0]), attrs.get("axis", -1), bool(attrs.get("largest", 1)))
            return [v, i]
        return [_act32(op, x, attrs, ins[1:])]


def _users(case):
    users = {}
    for i, n in enumerate(case.nodes):
        for s in n["inputs"]:
            if s:
                users.setdefault(s, []).append(i)
    return users


def _scalar_const(case, name):
    a = case.inits.get(name)
    return None if a is None or a.dtype != F or a.size != 1 else F(a.reshape(-1)[0])


def _reference_matmul_fusions(case):
    """{node index: replacement} for the two arithmetic-changing fusions of the reference (module docstring).  A replacement is ("skip",) for an
    absorbed MatMul or (alpha, bias name or None, a, b) for the Mul / Div / Add that becomes the FusedMatMul's output."""
    users, outs = _users(case), set(case.outputs)
    producer = {o: i for i, n in enumerate(case.nodes) for o in n["outputs"]}
    plan = {}
    for i, n in enumerate(case.nodes):
        if n["op"] != "MatMul":
            continue
        y = n["outputs"][0]
        if y in outs or len(users.get(y, [])) != 1:  # a fusion never removes a value somebody else reads
            continue
        u = case.nodes[users[y][0]]
        a, b = n["inputs"]
        if u["op"] in ("Mul", "Div"):  # fusions.rs:884-906: Mul takes the scalar on either side, Div on the right only
            lhs, rhs = u["inputs"]
            c = _scalar_const(case, rhs) if lhs == y else (_scalar_const(case, lhs) if u["op"] == "Mul" else None)
            if c is None or lhs == rhs:
                continue
            alpha = F(1.0) / c if u["op"] == "Div" else c
            if alpha == F(1.0):  # fusions.rs:951-954
                continue
            plan[i], plan[users[y][0]] = ("skip",), (float(alpha), None, a, b)
        elif u["op"] == "Add":  # fusions.rs:815-846
            other = u["inputs"][1] if u["inputs"][0] == y else u["inputs"][0]
            if other in case.inits and case.inits[other].ndim == 1 and other not in producer and other != y:
                plan[i], plan[users[y][0]] = ("skip",), (1.0, other, a, b)
    return plan


class ExpectedError(Exception):
    """The graph must be refused with this message (Case.expect["error"])."""


class _Canonical:
    """The graph as Graph::canonicalize must leave it: tests/fusion_rules.py applied to the case's nodes (`Constant` nodes become constants; Silu,
    Swish, Gelu and LayerNormalization idioms become those operators where the reference's rules fuse them)."""

    def __init__(self, case):
        from tests import fusion_rules as FR
        ranks = {name: len(dims) for name, dims in case.input_specs}
        self.nodes, self.inits, self.log = FR.rewrite(case.nodes, case.inits, case.outputs, ranks)
        self.outputs = case.outputs


def canonical(case):
    if getattr(case, "_canonical", None) is None:
        case._canonical = _Canonical(case)
    return case._canonical


def evaluate(case, binding=0, fused=True):
    """{value name: ndarray} of every value of the canonical graph, node by node.  fused=False: the --no-fuse expectation.  The load-time rewrite
    (`canonical`) applies in both modes: Graph::compile canonicalises whether or not its own fusions are on."""
    inputs = case.bindings[binding]
    case = canonical(case)
    vals = dict(case.inits)
    vals.update(inputs)
    plan = _reference_matmul_fusions(case) if fused else {}
    for i, n in enumerate(case.nodes):
        r = plan.get(i)
        if r == ("skip",):
            continue
        if r is not None:
            alpha, bias, a, b = r
            if bias is not None and vals[bias].size != vals[b].shape[-1]:
                raise ExpectedError("Cannot broadcast bias to output shape")
            node = {"op": "FusedMatMul", "attrs": {"alpha": alpha}}
            out = eval_node(node, [vals[a], vals[b]] + ([vals[bias]] if bias is not None else []))
        else:
            out = eval_node(n, [vals[s] if s else None for s in n["inputs"]])
        for name, v in zip(n["outputs"], out):
            if name:
                vals[name] = _narrow(v)  # (Shape and what is computed from it: int32 to the executor, so a graph output of that kind reads back as I32)
    return vals


# ------------------------------------------------------------------------------------------------ independent float64 evaluation
def _rnn64(op, ins, attrs):
    """ONNX GRU (linear_before_reset=1, gates z r h) / LSTM (gates i o f c) with the default activations, zero initial state, in float64."""
    x, w, r = (np.asarray(a, np.float64) for a in ins[:3])
    b = np.asarray(ins[3], np.float64) if len(ins) > 3 and ins[3] is not None else None
    direction = attrs.get("direction", "forward")
    seq, batch, _ = x.shape
    G = 3 if op == "GRU" else 4
    dirs, H = w.shape[0], w.shape[1] // G
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))
    y = np.zeros((seq, dirs, batch, H))
    h, c = np.zeros((dirs, batch, H)), np.zeros((dirs, batch, H))
    for d in range(dirs):
        backwards = direction == "reverse" or d == 1
        wb = b[d, :G * H] if b is not None else 0.0
        rb = b[d, G * H:] if b is not None else 0.0
        for t in (reversed(range(seq)) if backwards else range(seq)):
            gx, gh = x[t] @ w[d].T + wb, h[d] @ r[d].T + rb
            if op == "GRU":
                z, rr = sg(gx[:, :H] + gh[:, :H]), sg(gx[:, H:2 * H] + gh[:, H:2 * H])
                cand = np.tanh(gx[:, 2 * H:] + rr * gh[:, 2 * H:])
                h[d] = (1.0 - z) * cand + z * h[d]
            else:
                g = gx + gh
                i, o, f = sg(g[:, :H]), sg(g[:, H:2 * H]), sg(g[:, 2 * H:3 * H])
                c[d] = f * c[d] + i * np.tanh(g[:, 3 * H:])
                h[d] = o * np.tanh(c[d])
            y[t, d] = h[d]
    return [y, h.copy()] + ([c.copy()] if op == "LSTM" else [])


def evaluate64(case, binding=0, teacher=None):
    """Every value in float64 with numpy / torch-CPU only.  Integer-valued results (u8 codes, zero points, indices) cannot be carried in a
    different precision: they are computed here for the comparison and then replaced by `teacher`'s (the f32 interpreter's) values, so that one
    rounding tie does not spread.  Returns (values, ties): ties[name] is a boolean mask of the elements of an integer output whose float64
    decision is within `TIE_MARGIN` of flipping."""
    import torch
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    vals, ties = {}, {}
    for k, v in list(case.inits.items()) + list(case.bindings[binding].items()):
        vals[k] = v.astype(np.float64) if v.dtype == F else v
    for n in case.nodes:
        op, attrs = n["op"], n["attrs"]
        ins = [vals[s] if s else None for s in n["inputs"]]
        x = ins[0] if ins else None
        with np.errstate(all="ignore"):
            if op in LAYOUT_OPS:
                out = _layout_op(op, ins, attrs)
            elif op in ("Add", "Sub", "Mul", "Div"):
                out = [{"Add": np.add, "Sub": np.subtract, "Mul": np.multiply, "Div": reference_div}[op](ins[0], ins[1])]
            elif op in ("Conv", "ConvInteger"):
                w = ins[1].astype(np.float64)
                xx = x.astype(np.float64)
                if op == "ConvInteger":
                    xx = xx - float(ins[2])
                    if len(ins) > 3 and ins[3] is not None:
                        w = w - np.asarray(ins[3], np.float64).reshape(-1, *([1] * (w.ndim - 1)))
                nsp = x.ndim - 2
                pads = list(attrs.get("pads", [0] * (2 * nsp)))
                xp = np.pad(xx, [(0, 0), (0, 0)] + [(pads[k], pads[k + nsp]) for k in range(nsp)])
                conv = torch.nn.functional.conv1d if nsp == 1 else torch.nn.functional.conv2d
                b = T(ins[2]) if op == "Conv" and len(ins) > 2 and ins[2] is not None else None
                y = conv(T(xp), T(w), b, stride=tuple(attrs.get("strides", [1] * nsp)), dilation=tuple(attrs.get("dilations", [1] * nsp)), groups=attrs.get("group", 1)).numpy()
                out = [np.rint(y).astype(np.int32) if op == "ConvInteger" else y]
            elif op == "Cast":
                out = [x.astype(np.float64) if attrs["to"] == ow.FLOAT else np.trunc(x).astype(np.int64)]
            elif op == "Equal":
                out = [(ins[0] == ins[1]).astype(np.int32)]
            elif op == "Where":
                out = [np.where(np.asarray(ins[0]) != 0, ins[1], ins[2])]
            elif op == "Expand":
                out = [np.array(np.broadcast_to(x, np.broadcast_shapes(x.shape, tuple(int(d) for d in ins[1]))))]
            elif op == "ConstantOfShape":
                fill = np.asarray(attrs["value"]).reshape(-1)[0] if attrs.get("value") is not None else np.float64(0)
                out = [np.full([int(d) for d in x], fill, np.float64 if np.asarray(fill).dtype.kind == "f" else np.int64)]
            elif op in ("GRU", "LSTM"):
                out = _rnn64(op, ins, attrs)
            elif op == "DynamicQuantizeLinear":  # the ONNX definition
                lo, hi = min(0.0, float(x.min())), max(0.0, float(x.max()))
                s = (hi - lo) / 255.0
                zf = np.clip(-lo / s, 0, 255) if s else 0.0
                z = np.rint(zf)
                qf = x / s + z if s else np.zeros_like(x)
                out = [np.clip(np.rint(qf), 0, 255).astype(np.uint8), np.float64(s), np.uint8(z)]
                ties[n["outputs"][0]] = np.abs(np.abs(qf - np.floor(qf)) - 0.5) < TIE_MARGIN * (1.0 + np.abs(qf))
                ties[n["outputs"][2]] = np.asarray(abs(abs(zf - np.floor(zf)) - 0.5) < TIE_MARGIN * (1.0 + abs(zf)))
            elif op == "MatMul":
                out = [np.matmul(ins[0], ins[1])]
            elif op == "Gemm":
                a = ins[0].T if attrs.get("transA", 0) else ins[0]
                b = ins[1].T if attrs.get("transB", 0) else ins[1]
                y = attrs.get("alpha", 1.0) * (a @ b)
                out = [y + attrs.get("beta", 1.0) * ins[2] if len(ins) > 2 and ins[2] is not None else y]
            elif op == "LayerNormalization":
                a = attrs.get("axis", -1) % x.ndim
                ax = tuple(range(a, x.ndim))
                mu = x.mean(axis=ax, keepdims=True)
                var = ((x - mu) ** 2).mean(axis=ax, keepdims=True)
                y = (x - mu) / np.sqrt(var + float(F(attrs.get("epsilon", 1e-5)))) * ins[1].reshape(x.shape[a:])
                out = [y + ins[2].reshape(x.shape[a:]) if len(ins) > 2 and ins[2] is not None else y]
            elif op == "Softmax":
                a = attrs.get("axis", -1)
                e = np.exp(x - x.max(axis=a, keepdims=True))
                out = [e / e.sum(axis=a, keepdims=True)]
            elif op in ("MaxPool", "AveragePool"):
                k, s, p = attrs["kernel_shape"], attrs.get("strides", [1, 1]), attrs.get("pads", [0, 0, 0, 0])
                assert p[0] == p[2] and p[1] == p[3]
                if op == "MaxPool":
                    out = [torch.nn.functional.max_pool2d(T(x), tuple(k), tuple(s), (p[0], p[1])).numpy()]
                else:
                    out = [torch.nn.functional.avg_pool2d(T(x), tuple(k), tuple(s), (p[0], p[1]), count_include_pad=False).numpy()]
            elif op == "GlobalAveragePool":
                out = [x.mean(axis=tuple(range(2, x.ndim)), keepdims=True)]
            elif op == "ReduceSum":
                out = [x.sum(axis=tuple(int(a) for a in ins[1]), keepdims=bool(attrs.get("keepdims", 1)))]
            elif op == "ReduceMean":
                out = [x.mean(axis=tuple(attrs["axes"]) if "axes" in attrs else tuple(int(a) for a in ins[1]), keepdims=bool(attrs.get("keepdims", 1)))]
            elif op == "Tanh":
                out = [np.tanh(x)]
            elif op == "ArgMax":
                a = attrs.get("axis", 0)
                srt = np.sort(x, axis=a)
                gap = np.take(srt, [-1], axis=a) - np.take(srt, [-2], axis=a)
                idx = np.expand_dims(np.argmax(x, axis=a), a).astype(np.int32)
                ties[n["outputs"][0]] = gap < TIE_MARGIN if attrs.get("keepdims", 1) else np.squeeze(gap < TIE_MARGIN, a)
                out = [idx if attrs.get("keepdims", 1) else np.squeeze(idx, a)]
            elif op == "TopK":
                k, a = int(np.asarray(ins[1]).ravel()[0]), attrs.get("axis", -1)
                order = np.argsort(-x if attrs.get("largest", 1) else x, axis=a, kind="stable")
                srt = np.take_along_axis(x, order, axis=a)
                gaps = np.abs(np.diff(srt, axis=a))
                pad = [(0, 0)] * x.ndim
                pad[a] = (1, 0)
                near_prev = np.pad(gaps, pad, constant_values=np.inf) < TIE_MARGIN
                pad[a] = (0, 1)
                near_next = np.pad(gaps, pad, constant_values=np.inf) < TIE_MARGIN
                tie = np.take(near_prev | near_next, np.arange(k), axis=a)
                out = [np.take(srt, np.arange(k), axis=a), np.take(order, np.arange(k), axis=a).astype(np.int32)]
                ties[n["outputs"][1]] = tie
            elif op == "Pad":
                nd = x.ndim
                pw = [(int(ins[1][d]), int(ins[1][nd + d])) for d in range(nd)]
                out = [np.pad(x, pw, mode="reflect") if attrs.get("mode", "constant") == "reflect" else np.pad(x, pw, constant_values=float(np.asarray(ins[2]).reshape(-1)[0]) if len(ins) > 2 and ins[2] is not None else 0.0)]
            elif op == "Max":
                out = [np.maximum.reduce(np.broadcast_arrays(*ins))]
            elif op == "Mean":
                out = [sum(ins) / float(len(ins))]
            elif op in ("ReduceL2", "ReduceLogSumExp", "ReduceMax"):
                ax, kd = tuple(int(a) for a in ins[1]), bool(attrs.get("keepdims", 1))
                if op == "ReduceL2":
                    out = [np.sqrt((x * x).sum(axis=ax, keepdims=kd))]
                elif op == "ReduceMax":
                    out = [x.max(axis=ax, keepdims=kd)]
                else:
                    mx = x.max(axis=ax, keepdims=True)
                    r = np.log(np.exp(x - mx).sum(axis=ax, keepdims=True)) + mx
                    out = [r if kd else np.squeeze(r, ax)]
            elif op == "GlobalMaxPool":
                out = [x.max(axis=tuple(range(2, x.ndim)), keepdims=True)]
            elif op == "CumSum":
                assert not attrs.get("exclusive", 0) and not attrs.get("reverse", 0)
                out = [np.cumsum(x, axis=int(np.asarray(ins[1]).reshape(-1)[0]))]
            elif op == "Trilu":
                kk = int(np.asarray(ins[1]).reshape(-1)[0]) if len(ins) > 1 and ins[1] is not None else 0
                out = [np.triu(x, kk) if attrs.get("upper", 1) else np.tril(x, kk)]
            elif op == "Tile":
                out = [np.tile(x, [int(r) for r in ins[1]])]
            elif op == "GatherElements":
                idx = np.asarray(ins[1]).astype(np.int64)
                a = attrs.get("axis", 0)
                out = [np.take_along_axis(x, np.where(idx < 0, idx + x.shape[a], idx), axis=a)]
            elif op == "DepthToSpace":
                bs = attrs["blocksize"]
                n_, c_, h_, w_ = x.shape
                assert attrs.get("mode", "DCR") == "DCR"
                out = [x.reshape(n_, bs, bs, c_ // (bs * bs), h_, w_).transpose(0, 3, 4, 1, 5, 2).reshape(n_, c_ // (bs * bs), h_ * bs, w_ * bs)]
            elif op == "Resize":
                out = [_resize_nearest_x2(x, ins, attrs)]
            elif op == "Constant":
                v = np.asarray(attrs["value"])
                out = [v.astype(np.float64) if v.dtype == F else v]
            elif op == "Erf":
                out = [torch.erf(T(x)).numpy()]
            elif op in ("Sqrt", "Neg", "Abs", "Exp"):
                out = [{"Sqrt": np.sqrt, "Neg": np.negative, "Abs": np.abs, "Exp": np.exp}[op](x)]
            elif op == "Pow":
                out = [np.power(x, ins[1])]
            elif op in ("InstanceNormalization", "BatchNormalization"):
                shp = (1, -1) + (1,) * (x.ndim - 2)
                eps = float(F(attrs.get("epsilon", 1e-5)))
                if op == "InstanceNormalization":
                    ax = tuple(range(2, x.ndim))
                    mu, var = x.mean(axis=ax, keepdims=True), x.var(axis=ax, keepdims=True)
                else:
                    mu, var = ins[3].reshape(shp), ins[4].reshape(shp)
                out = [(x - mu) / np.sqrt(var + eps) * ins[1].reshape(shp) + ins[2].reshape(shp)]
            elif op == "LogSoftmax":
                a = attrs.get("axis", -1)
                d = x - x.max(axis=a, keepdims=True)
                out = [d - np.log(np.exp(d).sum(axis=a, keepdims=True))]
            elif op in ("QuantizeLinear", "DequantizeLinear"):
                a = attrs.get("axis", 1)
                per_axis = np.asarray(ins[1]).size != 1
                shp = [1] * x.ndim
                if per_axis:
                    shp[a] = -1
                sc = np.asarray(ins[1], np.float64).reshape(shp)
                zp = np.asarray(ins[2]).astype(np.float64).reshape(shp) if len(ins) > 2 and ins[2] is not None else 0.0
                if op == "QuantizeLinear":
                    dt = np.asarray(ins[2]).dtype
                    lo, hi = (0, 255) if dt == np.uint8 else (-128, 127)
                    qf = x / sc
                    out = [np.clip(np.rint(qf) + zp, lo, hi).astype(dt)]
                    ties[n["outputs"][0]] = np.abs(np.abs(qf - np.floor(qf)) - 0.5) < TIE_MARGIN * (1.0 + np.abs(qf))
                else:
                    out = [(np.asarray(x).astype(np.float64) - zp) * sc]
            else:
                one = 1.0
                sig = lambda v: one / (one + np.exp(-v))
                if op == "Relu":
                    out = [np.fmax(x, 0.0)]  # f32::max semantics (rten-vecmath/src/relu.rs): Relu(NaN) = 0
                elif op == "Gelu":
                    out = [0.5 * x * (1.0 + torch.erf(T(x) / np.sqrt(2.0)).numpy())]
                elif op == "Sigmoid":
                    out = [sig(x)]
                elif op == "Silu":
                    out = [x * sig(x)]
                elif op == "Swish":
                    out = [x * sig(x * float(F(attrs.get("alpha", 1.0))))]
                elif op == "HardSigmoid":
                    out = [np.clip(float(F(attrs.get("alpha", 0.2))) * x + float(F(attrs.get("beta", 0.5))), 0.0, 1.0)]
                elif op == "HardSwish":
                    out = [x * np.clip(x / 6.0 + 0.5, 0.0, 1.0)]
                elif op == "LeakyRelu":
                    out = [np.where(x < 0, x * float(F(attrs.get("alpha", 0.01))), x)]
                elif op == "Elu":
                    out = [np.where(x >= 0, x, float(F(attrs.get("alpha", 1.0))) * (np.exp(x) - 1.0))]
                elif op == "Clip":
                    lo = ins[1] if len(ins) > 1 and ins[1] is not None else -np.inf
                    hi = ins[2] if len(ins) > 2 and ins[2] is not None else np.inf
                    out = [np.minimum(np.maximum(x, lo), hi)]
                else:
                    raise KeyError(op)
        for name, v in zip(n["outputs"], out):
            if not name:
                continue
            v = np.asarray(v)
            if v.dtype.kind in "iu" and teacher is not None and op not in LAYOUT_OPS:
                vals[name + "#f64"] = v
                v = teacher[name]
            vals[name] = v
    return vals, ties


F64_BOUND = 2.34e-5  # |f32 oracle - float64| / (1 + |float64|) over the corpus stays below this (measured in tests/test_graph_fuzz_oracle.py)
TIE_MARGIN = F64_BOUND  # a float64 decision (rounding, arg-max, top-k order) closer than this to flipping is not compared


# ------------------------------------------------------------------------------------------------ builder
class Builder:
    """Builds a Case node by node; every node is evaluated at once on the f32 oracle so that later nodes can be shaped after its result."""

    def __init__(self, name, seed):
        self.case = Case(name)
        self.rng = np.random.default_rng(seed)
        self.v = {}       # name -> ndarray, first binding
        self.made_by = {}  # name -> op type of the producing node
        self.k = 0
        self.alt = None   # optional second binding: {input name: ndarray}
        self.opset = 17
        self.later_k = 0  # glue_later's rotation

    def fresh(self, stem):
        self.k += 1
        return f"{stem}{self.k}"

    def data(self, shape, scale=1.0):
        """U[-scale, scale) float32."""
        return ((self.rng.random(shape, dtype=np.float32) * F(2.0) - F(1.0)) * F(scale)).astype(F)

    def inp(self, shape, dims=None, arr=None):
        name = self.fresh("in")
        a = self.data(shape) if arr is None else arr
        self.case.input_specs.append((name, list(dims if dims is not None else a.shape)))
        self.case.bindings[0][name] = a
        self.v[name] = a
        self.made_by[name] = "input"
        return name

    def const(self, arr, stem="c"):
        name = self.fresh(stem)
        a = np.asarray(arr)
        self.case.inits[name] = a
        self.v[name] = a
        return name

    def cf(self, shape, scale=1.0):
        return self.const(self.data(shape, scale))

    def ci(self, values):
        return self.const(np.asarray(values, np.int64), "i")

    def node(self, op, inputs, nout=1, outputs=None, **attrs):
        outs = outputs or [self.fresh(op.lower()[:4] + "_") for _ in range(nout)]
        n = {"op": op, "inputs": list(inputs), "outputs": list(outs), "attrs": attrs, "name": self.fresh("n_" + op)}
        res = eval_node(n, [self.v[s] if s else None for s in inputs])
        assert len(res) >= len(outs), (op, len(res))
        for o, r in zip(outs, res):
            if o:
                assert r.size <= MAX_ELEMS, (op, r.shape)
                self.v[o] = r
                self.made_by[o] = op
        self.case.nodes.append(n)
        return outs[0] if len(outs) == 1 else outs

    def out(self, name):
        self.case.outputs.append(name)

    def row(self, row, folded=0, kinds=()):
        e = self.case.expect
        e["rows"].append(row)
        e["folded"] += folded
        e["kinds"] += list(kinds)

    def finish(self):
        c = self.case
        assert c.outputs, c.name
        if self.opset >= 18:  # ReduceMean-18 has no `axes` attribute: once a motif or the glue has raised the opset, every ReduceMean takes its axes as an input
            for n in c.nodes:
                if n["op"] == "ReduceMean" and "axes" in n["attrs"]:
                    n["inputs"] = [n["inputs"][0], self.ci(n["attrs"].pop("axes"))]
        elem = {np.dtype(np.float32): ow.FLOAT, np.dtype(np.uint8): ow.UINT8, np.dtype(np.int8): ow.INT8, np.dtype(np.int32): ow.INT32, np.dtype(np.int64): ow.INT64}
        nodes = [ow.node(n["op"], n["inputs"], n["outputs"], name=n["name"], **n["attrs"]) for n in c.nodes]
        ins = [ow.value_info(name, elem[c.bindings[0][name].dtype], dims) for name, dims in c.input_specs]
        outs = [ow.value_info(o, elem[self.v[o].dtype], list(self.v[o].shape) if self.alt is None else []) for o in c.outputs]
        c.onnx = ow.model(nodes, ins, outs, [ow.tensor(k, a) for k, a in c.inits.items()], opset=self.opset, name=c.name)
        if self.alt is not None:
            c.bindings.append(self.alt)
        c.expect["kinds"] = sorted(c.expect["kinds"])
        # what the loader's canonical form must be, by the reference's rules: the operators of the rewritten node list, or None where the rules rewrite nothing
        import collections
        can = canonical(c)
        c.expect["canonical"] = sorted(collections.Counter(n["op"] for n in can.nodes).items()) if len(can.nodes) != len(c.nodes) else None
        c.expect["canonical_nodes"] = len(can.nodes)
        folded = sum(1 for f, _ in can.log if f == "ConstantPropagation")  # DequantizeLinear nodes over initializers, and the initializers left behind
        c.expect["folded_dequantize"] = (folded, len(can.inits)) if folded else None
        return c


# ------------------------------------------------------------------------------------------------ motifs
# Every motif takes the builder, a variant name and a float32 source value of any shape (it derives its own operand from it with inert operators, so
# motifs chain), emits its nodes, records its row and returns the values a later motif or a graph output may read.

def _to4d(b, src, c, hw):
    """[1, c, hw, hw] f32 derived from `src` (flatten, slice or tile by Concat, reshape): nothing here is a fusion head or tail."""
    need = c * hw * hw
    flat = b.node("Reshape", [src, b.ci([-1])])
    while b.v[flat].size < need:
        flat = b.node("Concat", [flat, flat], axis=0)
    cut = b.node("Slice", [flat, b.ci([0]), b.ci([need]), b.ci([0]), b.ci([1])])
    return b.node("Reshape", [cut, b.ci([1, c, hw, hw])])


def _to2d(b, src, m, k):
    need = m * k
    flat = b.node("Reshape", [src, b.ci([-1])])
    while b.v[flat].size < need:
        flat = b.node("Concat", [flat, flat], axis=0)
    cut = b.node("Slice", [flat, b.ci([0]), b.ci([need]), b.ci([0]), b.ci([1])])
    return b.node("Reshape", [cut, b.ci([m, k])])


def m_conv(b, variant, src):
    r = b.rng
    C, O, HW = 4, 4, int(r.integers(5, 9))
    row = "conv/" + variant
    if variant == "conv1d_add":
        flat = _to2d(b, src, 1, 4 * 12)
        x = b.node("Reshape", [flat, b.ci([1, 4, 12])])
        res = b.node("Sub", [x, b.cf((1, 4, 12))])
        y = b.node("Conv", [x, b.cf((4, 4, 3), 0.4), b.cf((4,))], kernel_shape=[3], pads=[1, 1], strides=[1], dilations=[1])
        s = b.node("Add", [y, res])
        z = b.node("Relu", [s])
        b.row(row, 2, ["Conv+Add+Relu"])  # the step claims both; a 1-D convolution then runs them as separate launches
        return [z]
    if variant == "conv1d_default_attrs":  # no attribute at all: the constant weight's rank says that the node is 1-D
        flat = _to2d(b, src, 1, 4 * 12)
        x = b.node("Reshape", [flat, b.ci([1, 4, 12])])
        z = b.node("Relu", [b.node("Conv", [x, b.cf((4, 4, 3), 0.4), b.cf((4,))])])
        b.row(row, 1, ["Conv+Relu"])
        return [z]
    x = _to4d(b, src, C, HW)
    groups = {"grouped": 2, "depthwise": 4}.get(variant, 1)
    k = int(r.choice([1, 3]))
    w = b.cf((O, C // groups, k, k), 0.4)
    bias = b.cf((O,))
    conv = lambda xin, ww=w: b.node("Conv", [xin, ww, bias], kernel_shape=[k, k], pads=[k // 2] * 4, strides=[1, 1], group=groups)
    if variant in ("res_ready", "grouped", "depthwise"):
        res = b.node("Sub", [x, b.cf((1, C, HW, HW))])
        y = conv(x)
        s = b.node("Add", [y, res] if r.integers(2) else [res, y])
        z = b.node("Relu", [s])
        b.row(row, 2, ["Conv+Add+Relu"])
        return [z]
    if variant == "res_after":  # the residual's producer stands after the convolution: ready_before is false, nothing is claimed
        y = conv(x)
        res = b.node("Sub", [x, b.cf((1, C, HW, HW))])
        s = b.node("Add", [y, res])
        z = b.node("Relu", [s])
        b.row(row, 0)
        return [z]
    if variant == "two_convs_one_add":  # only the later convolution claims the Add
        y1 = conv(x)
        y2 = conv(x, b.cf((O, C, k, k), 0.4))
        s = b.node("Add", [y1, y2])
        z = b.node("Relu", [s])
        b.row(row, 2, ["Conv+Add+Relu"])
        return [z]
    if variant == "add_same":
        y = conv(x)
        s = b.node("Add", [y, y])
        z = b.node("Relu", [s])
        b.row(row, 0)
        return [z]
    if variant in ("res_const_1o11", "res_const_o11", "res_scalar"):  # claimed at load, run as Conv, broadcasting Add, Relu
        shape = {"res_const_1o11": (1, O, 1, 1), "res_const_o11": (O, 1, 1), "res_scalar": ()}[variant]
        y = conv(x)
        s = b.node("Add", [y, b.cf(shape)])
        z = b.node("Relu", [s])
        b.row(row, 2, ["Conv+Add+Relu"])
        return [z]
    if variant == "out_second_reader":
        y = conv(x)
        z = b.node("Relu", [y])
        t = b.node("Sub", [y, b.cf((1, O, 1, 1))])
        b.row(row, 0)
        return [z, t]
    if variant == "out_is_graph_output":
        y = conv(x)
        b.out(y)
        z = b.node("Relu", [y])
        b.row(row, 0)
        return [z]
    if variant == "add_is_output_relu_after":
        res = b.node("Sub", [x, b.cf((1, C, HW, HW))])
        y = conv(x)
        s = b.node("Add", [y, res])
        b.out(s)
        z = b.node("Relu", [s])
        b.row(row, 1, ["Conv+Add"])
        return [z]
    if variant == "relu":
        z = b.node("Relu", [conv(x)])
        b.row(row, 1, ["Conv+Relu"])
        return [z]
    assert variant.startswith("act_"), variant
    kind = variant[4:]
    y = conv(x)
    attrs, extra = {}, []
    if kind == "Swish":
        attrs = {"alpha": 1.702}
    elif kind == "HardSigmoid":
        attrs = {"alpha": 0.25, "beta": 0.5}
    elif kind in ("LeakyRelu", "Elu"):
        attrs = {"alpha": 0.3}
    elif kind == "Clip":
        extra = [b.const(np.array(-0.25, F)), b.const(np.array(0.5, F))]
    z = b.node(kind, [y] + extra, **attrs)
    b.row(row, 1, ["Conv+" + kind])
    return [z]


CONV_VARIANTS = ["res_ready", "res_after", "two_convs_one_add", "add_same", "res_const_1o11", "res_const_o11", "res_scalar", "conv1d_add",
                 "out_second_reader", "out_is_graph_output", "add_is_output_relu_after", "relu", "grouped", "depthwise"] + ["act_" + k for k in ACT_KINDS]


def m_matmul(b, variant, src):
    r = b.rng
    row = "matmul/" + variant
    big_k = variant.endswith("_k300")
    base = variant[:-5] if big_k else variant
    K = 300 if big_k else int(r.choice([24, 64, 256]))
    M, N = int(r.integers(2, 7)), int(r.choice([8, 20, 33]))
    if base == "one_row_bias":
        M = 1
    a = _to2d(b, src, M, K)
    if base == "batched_3d_bias":
        a2 = _to2d(b, src, 3 * M, K)
        a = b.node("Reshape", [a2, b.ci([3, M, K])])
    w = b.cf((K, N), 0.3)
    if base == "div_left":  # a product of non-negative factors stays away from zero, where c / y is ill-conditioned
        a, w = b.node("Mul", [a, a]), b.const(np.abs(b.v[w]) + F(0.05))
    y = b.node("MatMul", [a, w])
    differ = "the reference's FusedMatMul rounds differently from MatMul followed by the scalar operator / the bias Add (tests/graph_fuzz.py docstring)"
    if base in ("mul_right_pow2", "mul_right_np2", "div_right_pow2", "div_right_np2", "mul_left_np2"):
        c = b.const(np.array({"pow2": 0.125, "np2": 0.3}[base.rsplit("_", 1)[1]], F).reshape(() if r.integers(2) else (1,)))
        op = "Div" if base.startswith("div") else "Mul"
        z = b.node(op, [c, y] if base == "mul_left_np2" else [y, c])
        b.row(row, 1, ["FusedMatMul"])
        if "np2" in base:
            b.case.expect["modes_differ"] = differ
        return [z]
    if base == "div_left":  # c / MatMul is no scaling of the product
        z = b.node("Div", [b.const(np.array(0.3, F)), y])
        b.row(row, 0)
        return [z]
    if base == "div_then_mul":  # the Div becomes alpha, the Mul stays
        d = b.node("Div", [y, b.const(np.array(3.0, F))])
        z = b.node("Mul", [d, b.const(np.array(0.7, F))])
        b.row(row, 1, ["FusedMatMul"])
        b.case.expect["modes_differ"] = differ
        return [z]
    if base in ("bias_1d", "one_row_bias", "batched_3d_bias", "bias_1d_left"):
        bias = b.cf((N,))
        s = b.node("Add", [bias, y] if base == "bias_1d_left" else [y, bias])
        b.row(row, 1, ["FusedMatMul"])
        b.case.expect["modes_differ"] = differ
        return [s]
    if base in ("bias_gelu", "bias_relu", "bias_act"):
        s = b.node("Add", [y, b.cf((N,))])
        kind = {"bias_gelu": "Gelu", "bias_relu": "Relu", "bias_act": str(r.choice(["Sigmoid", "Silu", "HardSwish", "Elu"]))}[base]
        z = b.node(kind, [s])
        b.row(row, 2, ["FusedMatMul+" + kind])
        b.case.expect["modes_differ"] = differ
        return [z]
    if base == "act_no_bias":
        z = b.node("Sigmoid", [y])
        b.row(row, 1, ["FusedMatMul+Sigmoid"])
        return [z]
    if base == "bias_1xn":  # a [1, N] constant is no bias vector: MatMul, Add
        s = b.node("Add", [y, b.cf((1, N))])
        b.row(row, 0)
        return [s]
    if base == "bias_nonconst":
        bias = b.node("Sub", [b.cf((N,)), b.cf((N,))])
        s = b.node("Add", [y, bias])
        b.row(row, 0)
        return [s]
    if base == "bias_len_mismatch":  # a constant [1]: the Add broadcasts it, the FusedMatMul refuses it
        s = b.node("Add", [y, b.cf((1,))])
        b.row(row, 1, ["FusedMatMul"])
        b.case.expect["error"] = {"fused": "Cannot broadcast bias to output shape", "nofuse": None}
        return [s]
    if base == "read_twice":
        s = b.node("Add", [y, b.cf((N,))])
        t = b.node("Sub", [y, b.cf((N,))])
        b.row(row, 0)
        return [s, t]
    raise KeyError(variant)


MATMUL_VARIANTS = ["mul_right_pow2", "mul_right_np2", "div_right_pow2", "div_right_np2", "mul_left_np2", "div_left", "div_then_mul", "bias_1d", "bias_1d_left",
                   "bias_1d_k300", "mul_right_np2_k300", "mul_left_np2_k300", "bias_gelu", "bias_relu", "bias_act", "bias_gelu_k300", "act_no_bias", "bias_1xn",
                   "bias_nonconst", "bias_len_mismatch", "batched_3d_bias", "one_row_bias", "one_row_bias_k300", "read_twice"]


def m_gemm(b, variant, src):
    r = b.rng
    M, K, N = int(r.integers(2, 6)), int(r.choice([16, 300])), int(r.choice([8, 21]))
    if variant == "one_row":
        M = 1
    ta, tb = variant in ("trans_a", "trans_ab"), variant in ("trans_b", "trans_ab", "alpha_beta_matrix")
    a = _to2d(b, src, K, M) if ta else _to2d(b, src, M, K)
    w = b.cf((N, K) if tb else (K, N), 0.3)
    attrs = {"transA": int(ta), "transB": int(tb)}
    ins = [a, w]
    if variant == "alpha_beta_matrix":
        attrs.update(alpha=0.5, beta=0.75)
        ins.append(b.cf((M, N)))
    elif variant != "no_c":
        ins.append(b.cf((N,)))
    y = b.node("Gemm", ins, **attrs)
    b.row("gemm/" + variant, 0)
    return [y]


GEMM_VARIANTS = ["vector_c", "trans_a", "trans_b", "trans_ab", "alpha_beta_matrix", "no_c", "one_row"]


def m_add_ln(b, variant, src):
    r = b.rng
    R, Cc = int(r.integers(2, 6)), int(r.choice([10, 64, 100]))
    row = "add_ln/" + variant
    if variant == "add_out_is_scale":  # the Add's result is read twice by the LayerNormalization: not a sole reader
        x = _to2d(b, src, 1, Cc)
        x1 = b.node("Reshape", [x, b.ci([Cc])])
        s = b.node("Add", [x1, b.cf((Cc,))])
        y = b.node("LayerNormalization", [s, s], axis=-1, epsilon=1e-5)
        b.row(row, 0)
        return [y]
    x = _to2d(b, src, 2 * R, Cc)
    x = b.node("Reshape", [x, b.ci([2, R, Cc])])
    gamma, beta = b.cf((Cc,)), b.cf((Cc,))
    if variant == "axis_other":  # LayerNormalization over the two trailing axes: Add, LayerNormalization
        s = b.node("Add", [x, b.cf((2, R, Cc))])
        y = b.node("LayerNormalization", [s, b.cf((R, Cc)), b.cf((R, Cc))], axis=1, epsilon=1e-5)
        b.row(row, 0)
        return [y]
    other = b.cf((Cc,)) if variant == "bcast_add" else b.cf((2, R, Cc))
    s = b.node("Add", [x, other] if r.integers(2) else [other, x])
    y = b.node("LayerNormalization", [s, gamma] + ([] if variant == "no_bias" else [beta]), axis=-1, epsilon=1e-12 if r.integers(2) else 1e-5)
    if variant == "add_is_output":
        b.out(s)
        b.row(row, 0)
    else:
        b.row(row, 1, ["Add+LayerNormalization"])
    return [y]


ADD_LN_VARIANTS = ["axis_last", "axis_other", "bcast_add", "add_out_is_scale", "no_bias", "add_is_output"]


def m_add_softmax(b, variant, src):
    r = b.rng
    R, Cc = int(r.integers(2, 6)), int(r.choice([7, 32, 130]))
    row = "add_softmax/" + variant
    x = _to2d(b, src, 3 * R, Cc)
    x = b.node("Reshape", [x, b.ci([3, R, Cc])])
    if variant == "other_axis":
        s = b.node("Add", [x, b.cf((3, R, Cc))])
        y = b.node("Softmax", [s], axis=1)
        b.row(row, 0)
        return [y]
    if variant == "last_axis":
        s = b.node("Add", [x, b.cf((3, R, Cc))])
    elif variant == "small_first":  # the step swaps the operands
        s = b.node("Add", [b.cf((Cc,)), x])
    elif variant == "bcast_both":  # [3, R, Cc] + [3, 1, Cc] is outside the fused kernel's forms; [3, 1, Cc] + [1, R, Cc] broadcasts both ways
        x1 = b.node("Slice", [x, b.ci([0]), b.ci([1]), b.ci([1]), b.ci([1])])
        s = b.node("Add", [x1, b.cf((1, R, Cc))])
    elif variant == "addend_of_higher_rank":  # [R, Cc] + [1, 1, Cc] is [1, R, Cc]: the sum takes the ADDEND's rank, so the fused kernel (output shaped like x) is not taken
        x2 = b.node("Reshape", [b.node("Slice", [x, b.ci([0]), b.ci([1]), b.ci([0]), b.ci([1])]), b.ci([R, Cc])])
        s = b.node("Add", [x2, b.cf((1, 1, Cc))])
    elif variant == "neg_inf_row":  # one row of the mask is all -inf: that row of the result is NaN
        mask = np.zeros((3, R, Cc), F)
        mask[1, 0, :] = -np.inf
        mask[2, R - 1, ::2] = -np.inf
        s = b.node("Add", [x, b.const(mask)])
    else:
        raise KeyError(variant)
    y = b.node("Softmax", [s], axis=-1)
    b.row(row, 1, ["AddSoftmax"])
    return [y]


ADD_SOFTMAX_VARIANTS = ["last_axis", "other_axis", "small_first", "bcast_both", "neg_inf_row", "addend_of_higher_rank"]


def m_views(b, variant, src):
    r = b.rng
    row = "views/" + variant
    A, B_ = int(r.integers(2, 5)), int(r.choice([6, 16, 40]))
    x = _to2d(b, src, A, B_)
    base = b.node("Sub", [x, b.cf((A, B_))])  # a pooled buffer of A * B_ floats
    if variant.startswith("chain"):
        depth = int(variant[5:])
        ops = [("Reshape", lambda v: [v, b.ci([1, A, B_])], {}), ("Flatten", lambda v: [v], {"axis": 2}), ("Unsqueeze", lambda v: [v, b.ci([0, 3])], {}),
               ("Squeeze", lambda v: [v, b.ci([0])], {})]
        v = base
        for d in range(depth):
            op, mk, attrs = ops[d] if d < 4 else ops[0]
            v = b.node(op, mk(v), **attrs)
            if d % 2 == 0:
                v = b.node("Identity", [v])
        y = b.node("Mul", [v, b.cf(b.v[v].shape)])
        b.row(row)
        return [y]
    if variant == "of_graph_input":
        g = b.inp((A, B_))
        v = b.node("Reshape", [g, b.ci([B_, A])])
        y = b.node("Sub", [v, b.cf((B_, A))])
        b.out(v)
        b.row(row)
        return [y]
    if variant == "of_initializer":
        v = b.node("Reshape", [b.cf((A, B_)), b.ci([B_, A])])
        b.out(v)
        xt = b.node("Reshape", [base, b.ci([B_, A])])
        y = b.node("Mul", [v, xt])
        b.row(row)
        return [y]
    if variant == "view_is_output":
        v = b.node("Flatten", [base], axis=0)
        b.out(v)
        y = b.node("Tanh", [base])
        b.row(row)
        return [y]
    if variant == "output_listed_twice":
        y = b.node("Tanh", [base])
        b.out(y)
        b.out(y)
        v = b.node("Reshape", [y, b.ci([-1])])
        b.out(v)
        b.out(v)
        b.row(row)
        return [b.node("Sub", [y, b.cf((B_,))])]
    if variant == "input_is_output":
        g = b.inp((A, B_))
        b.out(g)
        b.row(row)
        return [b.node("Mul", [g, base])]
    if variant == "read_after_base_dies":
        # v aliases `base`; Tanh is base's last other reader; `again` then asks the pool for a buffer of base's size while v is still to be read
        v = b.node("Reshape", [base, b.ci([B_, A])])
        t = b.node("Tanh", [base])
        again = b.node("Sub", [t, b.cf((A, B_))])
        more = b.node("Mul", [again, b.cf((A, B_))])
        w = b.node("Mul", [v, b.cf((B_, A))])
        b.out(w)
        b.row(row)
        return [more]
    if variant == "view_of_view_after_base_dies":
        v1 = b.node("Reshape", [base, b.ci([B_, A])])
        v2 = b.node("Unsqueeze", [v1, b.ci([0])])
        t = b.node("Tanh", [v1])  # v1's last reader: its hold on base goes, v2's must stay
        again = b.node("Sub", [t, b.cf((B_, A))])
        more = b.node("Mul", [again, b.cf((B_, A))])
        w = b.node("Mul", [v2, b.cf((1, B_, A))])
        b.out(w)
        b.row(row)
        return [more]
    if variant == "unread_view":
        b.node("Reshape", [base, b.ci([-1])])
        y = b.node("Tanh", [base])
        b.row(row)
        return [b.node("Sub", [y, b.cf((A, B_))])]
    if variant == "add_v_v":
        v = b.node("Reshape", [base, b.ci([B_, A])])
        y = b.node("Add", [v, v])
        b.row(row)
        return [y]
    if variant == "split_second_unread":
        h = B_ // 2
        p0, _ = b.node("Split", [base, b.ci([h, B_ - h])], nout=2, axis=1)
        b.row(row)
        return [b.node("Sub", [p0, b.cf((A, h))])]
    if variant == "topk_indices_unread":
        vals, _ = b.node("TopK", [base, b.ci([3])], nout=2, axis=-1, largest=1)
        b.row(row)
        return [b.node("Sub", [vals, b.cf((A, 3))])]
    if variant == "topk_values_unread":
        _, idx = b.node("TopK", [base, b.ci([3])], nout=2, axis=-1, largest=1)
        b.out(idx)
        am = b.node("ArgMax", [base], axis=1, keepdims=0)
        b.out(am)
        b.row(row)
        return [b.node("Tanh", [base])]
    if variant == "dql_scale_unread":
        x4 = _to4d(b, base, 4, 5)
        q, _, zp = b.node("DynamicQuantizeLinear", [x4], nout=3)
        wq = b.const(b.rng.integers(-64, 65, (3, 4, 1, 1)).astype(np.int8))
        acc = b.node("ConvInteger", [q, wq, zp], kernel_shape=[1, 1])
        b.out(acc)
        b.out(q)
        b.row(row)
        return [b.node("Tanh", [x4])]
    raise KeyError(variant)


VIEW_VARIANTS = ["chain2", "chain3", "chain4", "of_graph_input", "of_initializer", "view_is_output", "output_listed_twice", "input_is_output", "read_after_base_dies",
                 "view_of_view_after_base_dies", "unread_view", "add_v_v", "split_second_unread", "topk_indices_unread", "topk_values_unread", "dql_scale_unread"]


def m_int8(b, variant, src):
    """DynamicQuantizeLinear -> ConvInteger -> Cast -> Mul(x_scale * w_scale) (+ Add bias [1,O,1,1]) (+ Add residual) (+ Relu), small and unpadded."""
    r = b.rng
    row = "int8/" + variant
    C, O, HW = 4, 4, 6
    x = _to4d(b, src, C, HW)
    zero = b.const(np.zeros((), np.int8))
    q, xs, xz = b.node("DynamicQuantizeLinear", [x], nout=3)

    def chain(k, per_channel=False, bias=True, residual=None, relu=False):
        wq = b.const(r.integers(-64, 65, (O, C, k, k)).astype(np.int8))
        ws = b.const((r.random((1, O, 1, 1), dtype=np.float32) * F(0.02) + F(0.005)) if per_channel else np.array(0.0123, F))
        acc = b.node("ConvInteger", [q, wq, xz, zero], kernel_shape=[k, k], pads=[0, 0, 0, 0], strides=[1, 1])
        accf = b.node("Cast", [acc], to=ow.FLOAT)
        sc = b.node("Mul", [xs, ws])
        y = b.node("Mul", [accf, sc])
        folded, kind = 2 + (0 if per_channel else 1), "ConvIntegerToFloat"  # Cast, Mul; the scalar scale product moves into the staged quantizer
        if bias:
            y = b.node("Add", [y, b.cf((1, O, 1, 1))])
            folded, kind = folded + 1, kind + "+bias"
        if residual is not None:
            y = b.node("Add", [y, residual])
            folded, kind = folded + 1, kind + "+Add"
        if relu:
            y = b.node("Relu", [y])
            folded, kind = folded + 1, kind + "+Relu"
        return y, folded, kind
    if variant in ("scalar_scale", "per_channel_scale"):
        y, f, k = chain(1, per_channel=variant == "per_channel_scale", relu=True)
        b.row(row, f, [k])
        return [y]
    if variant == "residual_relu":
        res = b.node("Sub", [x, b.cf((1, C, HW, HW))])
        y, f, k = chain(1, residual=res, relu=True)
        b.row(row, f, [k])
        return [y]
    if variant == "one_quantizer_two_convs":  # two convolutions of one geometry read the codes; the scale feeds two Mul nodes
        y1, f1, k1 = chain(1, relu=True)
        y2, f2, k2 = chain(1, bias=False)
        b.row(row, f1 + f2, [k1, k2])
        return [b.node("Sub", [y1, y2])]
    if variant == "quantizer_input_read_elsewhere":
        y, f, k = chain(3)
        b.out(x)
        t = b.node("Tanh", [x])
        b.row(row, f, [k])
        return [y, t]
    if variant == "scale_read_by_second_mul":  # x_scale also scales an f32 tensor: that Mul is no scale product
        y, f, k = chain(1)
        t = b.node("Mul", [x, xs])
        b.row(row, f, [k])
        return [y, t]
    raise KeyError(variant)


INT8_VARIANTS = ["scalar_scale", "per_channel_scale", "residual_relu", "one_quantizer_two_convs", "quantizer_input_read_elsewhere", "scale_read_by_second_mul"]

# ---- exporter idioms the loader canonicalises (Graph::canonicalize) by the reference's rules (tests/fusion_rules.py).  A row says whether its idiom
#      fuses; what the canonical graph must be is computed from the rules (Case.expect["canonical"]), not from the row.
SQRT2 = np.sqrt(F(2.0))


def _gelu_idiom(b, x, form="(x*e)*h", half=0.5, sqrt2=SQRT2, inner="div", shape=(), x_erf=None, half_value=None):
    k = lambda v: b.const(np.full(shape, v, F))
    xe = x_erf or x
    s = b.node("Div", [xe, k(sqrt2)]) if inner == "div" else b.node("Mul", [xe, k(F(1.0) / F(sqrt2))])
    erf = b.node("Erf", [s])
    e = b.node("Add", [erf, k(1.0)])
    h = half_value or k(half)
    if form == "(x*e)*h":
        inner_v = b.node("Mul", [x, e])
        y = b.node("Mul", [inner_v, h])
    elif form == "h*(x*e)":
        inner_v = b.node("Mul", [x, e])
        y = b.node("Mul", [h, inner_v])
    elif form == "(x*h)*e":
        inner_v = b.node("Mul", [x, h])
        y = b.node("Mul", [inner_v, e])
    else:
        assert form == "x*(e*h)", form
        inner_v = b.node("Mul", [e, h])
        y = b.node("Mul", [x, inner_v])
    return y, erf, inner_v


GELU_FUSING = {"gelu_xe_h": {}, "gelu_h_xe": dict(form="h*(x*e)"), "gelu_xh_e": dict(form="(x*h)*e"), "gelu_x_eh": dict(form="x*(e*h)"), "gelu_inner_mul": dict(inner="mul"),
               "gelu_half_plus_9e-5": dict(half=0.5 + 9e-5), "gelu_half_minus_9e-5": dict(half=0.5 - 9e-5), "gelu_sqrt2_1.4142": dict(sqrt2=1.4142, form="(x*h)*e"),
               "gelu_consts_shape1": dict(shape=(1,))}
GELU_SPOILED = ["gelu_half_plus_2e-4", "gelu_half_minus_2e-4", "gelu_erf_read_twice", "gelu_inner_is_output", "gelu_x_differs", "gelu_x_is_product_scale_first",
                "gelu_half_not_const"]
SILU_FUSING = ["silu_x_sig", "silu_sig_x", "swish_alpha_rank0", "swish_alpha_shape1_sig_first"]
SILU_SPOILED = ["swish_alpha_vector", "silu_sig_read_twice", "silu_sig_of_other"]
LN_FUSING = {"ln_bias": {}, "ln_no_bias": dict(bias=False), "ln_bias_first": dict(bias_first=True), "ln_eps_first": dict(eps_first=True), "ln_scale_first": dict(scale_first=True),
             "ln_axes_input": dict(axes_input=True), "ln_axis_positive": dict(positive=True), "ln_keepdims0_rank1": dict(keepdims=0), "ln_pow_2.00005": dict(exponent=2.00005)}
LN_SPOILED = {"ln_axis_inner": dict(axes=[1]), "ln_pow_3": dict(exponent=3.0), "ln_scale_not_const": dict(scale_value=True), "ln_center_read_thrice": dict(),
              "ln_var_is_output": dict(), "ln_means_differ": dict(means_differ=True)}
IDIOM_VARIANTS = list(GELU_FUSING) + ["gelu_x_is_product"] + GELU_SPOILED + SILU_FUSING + SILU_SPOILED + list(LN_FUSING) + list(LN_SPOILED) + ["constant_node"]
IDIOM_MUST_NOT_FUSE = GELU_SPOILED + SILU_SPOILED + list(LN_SPOILED)
# Idioms the reference fuses although a constant is off its nominal value (inside the matcher's tolerance): the fused operator computes the NOMINAL function,
# which is then not the function the nodes spell (x ** 2.00005 of a negative number is NaN).  `evaluate64`, which evaluates the nodes as written, does not
# describe these values; tests/test_graph_fuzz_oracle.py leaves the idiom's result and everything computed from it out of its float64 comparison (the rest of
# the graph is compared as usual) and checks that the result itself does differ.
IDIOM_OFF_NOMINAL = ["gelu_half_plus_9e-5", "gelu_half_minus_9e-5", "ln_pow_2.00005"]  # (sqrt 2 written 1.4142 moves the result by 2e-6: compared like every other row)


def _ln_idiom(b, x, Cc, axes=(-1,), axes_input=False, keepdims=1, exponent=2.0, eps_first=False, scale_first=False, bias=True, bias_first=False, scale_value=False,
              means_differ=False, positive=False, rank=3):
    axes = [rank - 1] if positive else list(axes)
    if axes_input:
        b.opset = 18  # ReduceMean takes its axes as an input from opset 18 on
    mean = lambda v: b.node("ReduceMean", [v, b.ci(axes)], keepdims=keepdims) if axes_input else b.node("ReduceMean", [v], axes=axes, keepdims=keepdims)
    other = b.node("Tanh", [x]) if means_differ else x
    center = b.node("Sub", [x, mean(other)])
    var = mean(b.node("Pow", [center, b.const(np.array(exponent, F))]))
    eps = b.const(np.array(1e-5 if b.rng.integers(2) else 1e-12, F))
    std = b.node("Sqrt", [b.node("Add", [eps, var] if eps_first else [var, eps])])
    norm = b.node("Div", [center, std])
    scale = b.inp((Cc,)) if scale_value else b.const(b.data((Cc,)) + F(1.5))  # (a value computed from constants alone would be a constant to the reference)
    y = b.node("Mul", [scale, norm] if scale_first else [norm, scale])
    if bias:
        beta = b.cf((Cc,))
        y = b.node("Add", [beta, y] if bias_first else [y, beta])
    return y, center, var


def m_idiom(b, variant, src):
    r = b.rng
    row = "idiom/" + variant
    R, Cc = int(r.integers(2, 5)), int(r.choice([10, 33, 64]))
    to3 = lambda: b.node("Reshape", [_to2d(b, src, 2 * R, Cc), b.ci([2, R, Cc])])
    if variant in GELU_FUSING or variant in ("gelu_half_plus_2e-4", "gelu_half_minus_2e-4"):
        kw = GELU_FUSING[variant] if variant in GELU_FUSING else dict(half=0.5 + 2e-4 if "plus" in variant else 0.5 - 2e-4)
        y, _, _ = _gelu_idiom(b, to3(), **kw)
        outs = [y]
    elif variant in ("gelu_x_is_product", "gelu_x_is_product_scale_first"):  # a chain of four operands: the strict matcher decides (fuses the pattern's own bracketing only)
        x = to3()
        p = b.node("Mul", [x, b.node("Tanh", [x])])
        outs = [_gelu_idiom(b, p, form="(x*e)*h" if variant == "gelu_x_is_product" else "(x*h)*e")[0]]
    elif variant == "gelu_erf_read_twice":
        y, erf, _ = _gelu_idiom(b, to3())
        outs = [y, b.node("Tanh", [erf])]
    elif variant == "gelu_inner_is_output":
        y, _, inner = _gelu_idiom(b, to3())
        b.out(inner)
        outs = [y]
    elif variant == "gelu_x_differs":
        x = to3()
        outs = [_gelu_idiom(b, x, x_erf=b.node("Tanh", [x]))[0]]
    elif variant == "gelu_half_not_const":
        x = to3()
        outs = [_gelu_idiom(b, x, half_value=b.inp((1,), arr=np.array([0.5], F)))[0]]  # 0.5 as a graph input: a value, not a constant
    elif variant in SILU_FUSING + SILU_SPOILED:
        x = to3()
        if variant.startswith("swish"):
            alpha = {"swish_alpha_rank0": np.array(1.702, F), "swish_alpha_shape1_sig_first": np.array([0.75], F), "swish_alpha_vector": b.data((Cc,)) + F(1.5)}[variant]
            arg = b.node("Mul", [b.const(alpha), x] if variant != "swish_alpha_shape1_sig_first" else [x, b.const(alpha)])
        else:
            arg = b.node("Tanh", [x]) if variant == "silu_sig_of_other" else x
        s = b.node("Sigmoid", [arg])
        y = b.node("Mul", [s, x] if variant in ("silu_sig_x", "swish_alpha_shape1_sig_first") else [x, s])
        outs = [y] + ([b.node("Tanh", [s])] if variant == "silu_sig_read_twice" else [])
    elif variant in LN_FUSING or variant in LN_SPOILED:
        kw = dict(LN_FUSING[variant] if variant in LN_FUSING else LN_SPOILED[variant])
        if variant == "ln_axis_positive":  # the reference knows the rank of a graph input (its declared shape); see tests/fusion_rules.py
            x = b.inp((2, R, Cc))
        elif variant == "ln_keepdims0_rank1":  # [C] - mean with keepdims = 0 broadcasts a scalar: the same function, and the rules fuse it
            x = b.node("Reshape", [_to2d(b, src, 1, Cc), b.ci([Cc])])
            kw["rank"] = 1
        else:
            x = to3()
        y, center, var = _ln_idiom(b, x, Cc, **kw)
        outs = [y]
        if variant == "ln_center_read_thrice":
            outs.append(b.node("Tanh", [center]))
        if variant == "ln_var_is_output":
            b.out(var)
    elif variant == "constant_node":  # Constant nodes feeding an idiom (0.5 and sqrt 2) and a fusion tail (a MatMul's bias, Clip's bounds)
        kc = lambda a: b.node("Constant", [], value=np.asarray(a, F))
        x = _to2d(b, src, R, Cc)
        e = b.node("Add", [b.node("Erf", [b.node("Div", [x, kc(SQRT2)])]), kc(1.0)])
        g = b.node("Mul", [b.node("Mul", [x, e]), kc(0.5)])
        s = b.node("Add", [b.node("MatMul", [g, b.cf((Cc, 8), 0.3)]), kc(b.data((8,)))])
        outs = [b.node("Clip", [s, kc(-0.25), kc(0.5)])]
        b.row(row, 2, ["FusedMatMul+Clip"])
        return outs
    else:
        raise KeyError(variant)
    if variant in IDIOM_OFF_NOMINAL:
        b.case.expect["off_nominal"] = (b.case.expect["off_nominal"] or []) + [outs[0]]  # the idiom's result: what reads it is not compared in float64
    b.row(row)
    return outs


NORM_ACT_VARIANTS = [f"{n}_{a}" for n in ("in", "bn") for a in ("Relu",) + ACT_KINDS] + ["in_follower_read_twice", "bn_out_is_output", "logsoftmax_relu"]


def m_norm_act(b, variant, src):
    """InstanceNormalization / BatchNormalization followed by Relu or an activation with load-time parameters: one step (make_norm_step)."""
    r = b.rng
    row = "norm_act/" + variant
    C, HW = 4, int(r.integers(3, 7))
    x = _to4d(b, src, C, HW)
    gamma, beta = b.const(b.data((C,)) + F(1.5)), b.cf((C,))
    inorm = lambda: b.node("InstanceNormalization", [x, gamma, beta], epsilon=1e-5)
    bnorm = lambda: b.node("BatchNormalization", [x, gamma, beta, b.cf((C,)), b.const(np.abs(b.data((C,))) + F(0.5))], epsilon=1e-5)
    if variant == "in_follower_read_twice":  # the normalised value has two readers: no fusion
        y = inorm()
        b.row(row, 0)
        return [b.node("Relu", [y]), b.node("Tanh", [y])]
    if variant == "bn_out_is_output":
        y = bnorm()
        b.out(y)
        b.row(row, 0)
        return [b.node("Relu", [y])]
    if variant == "logsoftmax_relu":  # LogSoftmax takes no follower
        y = b.node("LogSoftmax", [x], axis=int(r.choice([1, -1])))
        b.row(row, 0)
        return [b.node("Relu", [y])]
    norm, kind = variant.split("_", 1)
    y = inorm() if norm == "in" else bnorm()
    attrs, extra = {}, []
    if kind == "Swish":
        attrs = {"alpha": 1.702}
    elif kind == "HardSigmoid":
        attrs = {"alpha": 0.25, "beta": 0.5}
    elif kind in ("LeakyRelu", "Elu"):
        attrs = {"alpha": 0.3}
    elif kind == "Clip":
        extra = [b.const(np.array(-0.25, F)), b.const(np.array(0.5, F))]
    z = b.node(kind, [y] + extra, **attrs)
    b.row(row, 1, [("InstanceNormalization+" if norm == "in" else "BatchNormalization+") + kind])
    return [z]


QDQ_VARIANTS = ["pair_u8", "pair_i8", "pair_per_axis", "zero_points_differ", "scales_differ", "codes_read_twice", "codes_is_output", "runtime_scale", "dql_over_initializers"]


def m_qdq(b, variant, src):
    """QuantizeLinear -> DequantizeLinear with equal constant parameters: one round-trip step (make_qdq_step); DequantizeLinear over initializers: folded at load."""
    r = b.rng
    row = "qdq/" + variant
    C, HW = 4, int(r.integers(3, 6))
    x = _to4d(b, src, C, HW)
    dt = np.int8 if variant == "pair_i8" else np.uint8
    zero = 3 if dt == np.int8 else 131
    if variant == "dql_over_initializers":  # counts in the canonical form: the node is gone, and the int8 codes with their zero point have no reader left
        wq = b.const(r.integers(-100, 101, (1, C, HW, HW)).astype(np.int8))
        w = b.node("DequantizeLinear", [wq, b.const(np.array(0.0173, F)), b.const(np.array(-5, np.int8))])
        b.row(row, 0)
        return [b.node("Mul", [x, w])]
    if variant == "pair_per_axis":
        mk_s, mk_z = lambda: b.const(np.array([0.011, 0.023, 0.017, 0.02], F)), lambda: b.const(np.array([120, 131, 128, 140], dt))
        attrs = {"axis": 1}
    else:
        mk_s, mk_z = lambda: b.const(np.array(0.0131, F)), lambda: b.const(np.array(zero, dt))
        attrs = {}
    qs, qz = mk_s(), mk_z()
    if variant == "runtime_scale":  # the scale is a graph input: each node is its own step
        qs = ds = b.inp((1,), arr=np.array([0.0131], F))
        dz = mk_z()
    else:
        ds = b.const(np.array(0.0137, F)) if variant == "scales_differ" else mk_s()  # equal constants under two names: compared by value
        dz = b.const(np.array(zero + 1, dt)) if variant == "zero_points_differ" else mk_z()
    q = b.node("QuantizeLinear", [x, qs, qz], **attrs)
    y = b.node("DequantizeLinear", [q, ds, dz], **attrs)
    outs = [y]
    if variant == "codes_read_twice":
        outs.append(b.node("Cast", [q], to=ow.FLOAT))
    if variant == "codes_is_output":
        b.out(q)
    if variant in ("pair_u8", "pair_i8", "pair_per_axis"):
        b.row(row, 1, ["QuantizeLinear+DequantizeLinear"])
    else:
        b.row(row, 0)
    return outs


# ---- attention: q / k / v [B, S|T, H] -> Reshape -> Transpose -> MatMul -> scale -> Add(mask) -> Softmax -> MatMul -> Transpose -> Reshape, which
#      plan_attention turns into one MultiHeadSdpa step (after one GEMM for the three projections when they are MatMul + Add of one input).
#      "big": hidden 128 = 2 heads x 64, S = T = 16 (the fused kernel); "small": hidden 16 = 2 x 8, S = 5, T = 7 from a second input (the general kernel).
ATTENTION_FUSING = {
    "separate_div_b11t_runtime": dict(scale="div", mask="b11t"),
    "merged_div_b11t_const": dict(proj="merged", scale="div", mask="b11t", mask_const=True),
    "merged_mul_b1st_runtime": dict(proj="merged", scale="mul", mask="b1st"),
    "small_noscale_b1st_const": dict(size="small", scale=None, mask="b1st", mask_const=True),
    "small_mul_const_first_11st_runtime": dict(size="small", scale="mul_first", mask="11st"),
    "separate_softmax_axis3_11st_const": dict(scale="div", mask="11st", mask_const=True, softmax_axis=3),
    "merged_explicit_reshape_st_runtime": dict(proj="merged", reshape="explicit", scale="div", mask="st"),
    "small_reshape_minus1_st_const": dict(size="small", reshape="minus1", scale="div", mask="st", mask_const=True),
    "separate_runtime_concat_nomask": dict(reshape="concat", scale="mul", mask=None),
    "runtime_head_mask": dict(scale="div", mask="1hst"),  # a per-head bias fed as an input: the plan fuses, the step runs the covered operators plainly
    "merged_mul_1hst_runtime": dict(proj="merged", scale="mul", mask="1hst"),  # ... on column blocks of the merged projection
    "small_minus1_div_1hst_runtime": dict(size="small", reshape="minus1", scale="div", mask="1hst"),  # ... heads spelled -1, a scale that is no power of two
}
ATTENTION_SPOILED = {
    "scores_read_twice": dict(spoil="scores"), "probabilities_are_output": dict(spoil="probs"), "k_transpose_is_output": dict(spoil="present_k"),
    "softmax_axis2": dict(softmax_axis=2), "k_perm_other": dict(spoil="k_perm"), "const_head_mask": dict(mask="1hst", mask_const=True, softmax_axis=3),
    "mask_after_scores": dict(mask="b11t", spoil="mask_late", softmax_axis=3),
    # q and k in 2 heads, v in ONE head of the full width: [B, 2, S, T] x [B, 1, T, H] broadcasts v over the heads.  The planner must refuse it (one head count
    # and one head size for q, k and v); run as written, the probabilities' MatMul then needs a batch prefix broadcast on one operand only, which the device
    # MatMul does not support -- a stated difference from the reference, which runs the graph (docs/KERNELS.md).  Pinned as an expected error of every mode.
    "v_head_count_differs": dict(spoil="v_heads"),
}
PARTIAL_BROADCAST_ERROR = "partial batch broadcasting is not supported by the device path"
ATTENTION_VARIANTS = list(ATTENTION_FUSING) + list(ATTENTION_SPOILED)


def m_attention(b, variant, src):
    kw = dict(ATTENTION_FUSING[variant] if variant in ATTENTION_FUSING else ATTENTION_SPOILED[variant])
    fusing = variant in ATTENTION_FUSING
    size, proj, reshape, spoil = kw.get("size", "big"), kw.get("proj", "separate"), kw.get("reshape", "zeros"), kw.get("spoil")
    scale, mask_form, mask_const, axis = (kw.get("scale") if fusing else None), kw.get("mask"), kw.get("mask_const", False), kw.get("softmax_axis", -1)
    B, h = 2, 2
    H, d, S, T = (128, 64, 16, 16) if size == "big" else (16, 8, 5, 7)
    shift = b.node("Reshape", [b.node("ReduceMean", [src], axes=list(range(b.v[src].ndim)), keepdims=1), b.ci([1])])  # the motif depends on its source value
    xq = b.node("Sub", [b.inp((B, S, H)), shift])
    xkv = xq if size == "big" else b.node("Sub", [b.inp((B, T, H)), shift])
    folded = 0
    if proj == "merged":
        lin = lambda x: b.node("Add", [b.node("MatMul", [x, b.cf((H, H), 0.15)]), b.cf((H,))])
        q, k, v = lin(xq), lin(xq), lin(xq)
        folded += 6 - 1  # three MatMul + Add pairs become one GEMM step
    else:
        q, k, v = xq, b.node("Tanh", [xkv]), b.node("Sub", [xkv, b.cf((H,))])

    def target(x, last):
        n = b.v[x].shape[1]
        if reshape == "explicit":
            return b.ci([B, n] + last)
        if reshape == "minus1" and len(last) == 2:
            return b.ci([0, 0, -1, last[1]])
        if reshape == "concat" and x == q and len(last) == 2:  # the dynamic-axes export: leading dims from Shape at run time
            shp = b.node("Shape", [x])
            dims = [b.node("Unsqueeze", [b.node("Gather", [shp, b.const(np.array(i, np.int64), "i")], axis=0), b.ci([0])]) for i in (0, 1)]
            return b.node("Concat", dims + [b.ci([last[0]]), b.ci([last[1]])], axis=0)
        return b.ci([0, 0] + last)
    split = lambda x, perm, last=None: b.node("Transpose", [b.node("Reshape", [x, target(x, last or [h, d])])], perm=perm)
    qh = split(q, [0, 2, 1, 3])
    kh = b.node("Transpose", [b.node("Reshape", [k, b.ci([0, 0, d, h])])], perm=[0, 3, 2, 1]) if spoil == "k_perm" else split(k, [0, 2, 3, 1])
    mask = None
    if mask_form:
        shape = {"b11t": (B, 1, 1, T), "b1st": (B, 1, S, T), "11st": (1, 1, S, T), "st": (S, T), "1hst": (1, h, S, T)}[mask_form]
        m = np.where(b.rng.random(shape) < 0.2, F(-1e4), F(0.0)).astype(F) + b.data(shape, 0.1)
        mask = b.const(m) if mask_const else b.inp(shape, arr=m)
    scores = cur = b.node("MatMul", [qh, kh])
    if spoil == "mask_late":  # the mask's producer stands after the scores
        mask = b.node("Tanh", [mask])
    c = np.array(np.sqrt(F(d)) if scale == "div" else F(1.0) / np.sqrt(F(d)), F)
    if scale == "div":
        cur = b.node("Div", [cur, b.const(c)])
    elif scale in ("mul", "mul_first"):
        cur = b.node("Mul", [cur, b.const(c)] if scale == "mul" else [b.const(c), cur])
    if mask:
        cur = b.node("Add", [cur, mask])
    probs = b.node("Softmax", [cur], axis=axis)
    vh = split(v, [0, 2, 1, 3], [1, H] if spoil == "v_heads" else None)
    ctx = b.node("MatMul", [probs, vh])
    merged_heads = b.node("Transpose", [ctx], perm=[0, 2, 1, 3])
    width = h * H if spoil == "v_heads" else H
    out = b.node("Reshape", [merged_heads, target(merged_heads, [width]) if reshape != "explicit" else b.ci([B, S, H])])
    outs = [out]
    if spoil == "scores":
        outs.append(b.node("Tanh", [scores]))
    if spoil == "probs":
        b.out(probs)
    if spoil == "present_k":
        b.out(kh)
    if fusing:  # every covered node but one: 3 x (Reshape, Transpose), 2 MatMul, Softmax, Transpose, Reshape (+ scale) (+ Add)
        folded += 11 + (scale is not None) + (mask is not None) - 1
        b.row("attention/" + variant, folded, ["FusedMatMul(QKV)", "MultiHeadSdpa(QKV column blocks)"] if proj == "merged" else ["MultiHeadSdpa"])
        if size == "small" and scale is not None:
            b.case.expect["modes_differ"] = "1 / sqrt(8) is no power of two: FusedMatMul's alpha against MatMul followed by the scalar operator"
    else:
        b.row("attention/" + variant, 0)
        if spoil == "v_heads":
            b.case.expect["error"] = {"fused": PARTIAL_BROADCAST_ERROR, "nofuse": PARTIAL_BROADCAST_ERROR, "device_only": True}
    return outs


MOTIFS = {"conv": (m_conv, CONV_VARIANTS), "matmul": (m_matmul, MATMUL_VARIANTS), "gemm": (m_gemm, GEMM_VARIANTS), "add_ln": (m_add_ln, ADD_LN_VARIANTS),
          "add_softmax": (m_add_softmax, ADD_SOFTMAX_VARIANTS), "views": (m_views, VIEW_VARIANTS), "int8": (m_int8, INT8_VARIANTS)}
HAND_ONLY_ROWS = ["shape/dynamic_batch_reshape", "conv/conv1d_default_attrs"]  # rows that have a minimal graph only, outside the seeds' walk of the table
OLD_ROWS = [f"{m}/{v}" for m, (_, vs) in MOTIFS.items() for v in vs] + HAND_ONLY_ROWS  # the table of the first 64 seeds: its order seeds the hand graphs
OLD_MOTIFS = dict(MOTIFS)
MOTIFS = dict(MOTIFS, idiom=(m_idiom, IDIOM_VARIANTS), attention=(m_attention, ATTENTION_VARIANTS), norm_act=(m_norm_act, NORM_ACT_VARIANTS), qdq=(m_qdq, QDQ_VARIANTS))
NEW_ROWS = [f"{m}/{v}" for m, (_, vs) in MOTIFS.items() if m not in OLD_MOTIFS for v in vs]  # walked by the seeds from 64 on
ROWS = OLD_ROWS + NEW_ROWS


# ------------------------------------------------------------------------------------------------ glue
# Inert operators only: nothing here is a fusion head (Conv, MatMul, Add, ConvInteger) and a fusion tail (Relu, an activation, Gelu, scalar Mul / Div,
# Add, LayerNormalization, Softmax, Cast) is emitted only behind a value that no head produced.
HEADS = ("Conv", "MatMul", "ConvInteger", "MatMulInteger", "Add", "Gemm")


def glue(b, src):
    r = b.rng
    x = b.v[src]
    choices = ["sub_bcast", "mul_bcast", "tanh", "transpose", "concat_slice", "split", "reduce"]
    if x.ndim == 4 and x.shape[2] >= 4 and x.shape[3] >= 4:
        choices += ["maxpool", "avgpool"]
    if b.made_by.get(src) not in HEADS + ("Mul", "Div", "Cast"):  # (a scalar Mul / Div may have become a FusedMatMul's result, which takes an activation)
        choices += ["activation", "relu"]
    pick = str(r.choice(choices))
    if pick in ("sub_bcast", "mul_bcast"):
        shape = list(x.shape)
        for d in range(len(shape)):
            if r.integers(2):
                shape[d] = 1
        shape = shape[int(r.integers(0, len(shape) + 1)) if shape else 0:] if r.integers(2) else shape
        if int(np.prod(shape, dtype=np.int64)) == 1 and pick == "mul_bcast":
            shape = list(x.shape)  # never a scalar Mul: that is the MatMul motif's tail
        c = b.cf(tuple(shape))
        op = "Sub" if pick == "sub_bcast" else "Mul"
        return b.node(op, [src, c] if r.integers(2) else [c, src])
    if pick == "tanh":
        return b.node("Tanh", [src])
    if pick == "transpose" and x.ndim >= 2:
        return b.node("Transpose", [src], perm=[int(p) for p in r.permutation(x.ndim)])
    if pick == "concat_slice" and x.ndim >= 1 and x.size * 2 <= MAX_ELEMS:
        ax = int(r.integers(x.ndim))
        cat = b.node("Concat", [src, b.node("Tanh", [src])], axis=ax)
        n = b.v[cat].shape[ax]
        lo = int(r.integers(0, n // 2))
        return b.node("Slice", [cat, b.ci([lo]), b.ci([lo + n // 2 + 1]), b.ci([ax]), b.ci([1])])
    if pick == "split" and x.ndim >= 1:
        ax = int(np.argmax(x.shape))
        n = x.shape[ax]
        if n >= 2:
            parts = b.node("Split", [src, b.ci([n // 2, n - n // 2])], nout=2, axis=ax)
            return parts[int(r.integers(2))] if r.integers(2) else b.node("Concat", [parts[1], parts[0]], axis=ax)
    if pick == "reduce" and x.ndim >= 2 and x.size >= 16:
        ax = int(r.integers(x.ndim))
        if r.integers(2):
            return b.node("ReduceSum", [src, b.ci([ax])], keepdims=1)
        return b.node("ReduceMean", [src], axes=[ax], keepdims=int(r.integers(2)) if x.ndim > 2 else 1)
    if pick == "maxpool":
        return b.node("MaxPool", [src], kernel_shape=[2, 2], strides=[2, 2], pads=[0, 0, 0, 0])
    if pick == "avgpool":
        return b.node("AveragePool", [src], kernel_shape=[3, 3], strides=[1, 1], pads=[1, 1, 1, 1])
    if pick == "activation":
        return b.node(str(r.choice(["Sigmoid", "HardSwish", "Elu", "LeakyRelu"])), [src])
    if pick == "relu":
        return b.node("Relu", [src])
    return b.node("Sub", [src, b.cf(x.shape)])


GLUE_LATER = ("instance_norm", "log_softmax", "pad_constant", "pad_reflect", "neg", "abs", "sqrt_abs", "exp", "max3", "mean3", "reduce_l2", "reduce_log_sum_exp",
              "reduce_max", "global_max_pool", "cum_sum", "trilu", "tile", "gather_elements", "depth_to_space", "resize_nearest")


def glue_later(b, src):
    """One inert operator of the later families (norm, math, reduce, index and sampling operators), evaluated by their restatements in tests/*_rules.py; falls
    back to the first table's glue where the value's shape does not suit the pick.  None of them is a fusion head; InstanceNormalization is followed by Tanh so
    that a later activation does not become its follower."""
    start = b.later_k  # the picks rotate, so that every one of them occurs in the corpus; the first one from here on that suits the value's shape is taken
    b.later_k += 1
    order = [GLUE_LATER[(start + j) % len(GLUE_LATER)] for j in range(len(GLUE_LATER))]
    if b.v[src].ndim == 4:  # 4-D values are rare in these graphs: the picks that need one go first there, rotating among themselves
        only4 = ("instance_norm", "global_max_pool", "depth_to_space", "resize_nearest")
        order = [only4[(start + j) % 4] for j in range(4)] + order
    for pick in order:
        y = _glue_later_pick(b, src, pick)
        if y is not None:
            return y
    return glue(b, src)


def _glue_later_pick(b, src, pick):
    r = b.rng
    x = b.v[src]
    four = x.ndim == 4
    small = x.size * 4 <= MAX_ELEMS
    if pick == "instance_norm" and four and x.shape[2] * x.shape[3] >= 2:
        C = x.shape[1]
        return b.node("Tanh", [b.node("InstanceNormalization", [src, b.const(b.data((C,)) + F(1.5)), b.cf((C,))], epsilon=1e-5)])
    if pick == "log_softmax" and x.ndim >= 1:
        return b.node("Tanh", [b.node("LogSoftmax", [src], axis=int(r.integers(-1, x.ndim)))])
    if pick == "pad_constant" and x.ndim >= 1 and small:
        pads = [int(v) for v in r.integers(0, 2, 2 * x.ndim)]
        return b.node("Pad", [src, b.ci(pads), b.const(np.array(0.25, F))], mode="constant")
    if pick == "pad_reflect" and x.ndim >= 2 and x.shape[-1] >= 3 and x.shape[-2] >= 3 and small:
        pads = [0] * (2 * x.ndim)
        pads[x.ndim - 2], pads[x.ndim - 1], pads[2 * x.ndim - 2], pads[2 * x.ndim - 1] = 1, 2, 2, 1
        return b.node("Pad", [src, b.ci(pads)], mode="reflect")
    if pick in ("neg", "abs", "exp"):
        return b.node(pick.capitalize(), [src])
    if pick == "sqrt_abs":
        return b.node("Sqrt", [b.node("Abs", [src])])
    if pick in ("max3", "mean3"):
        return b.node("Max" if pick == "max3" else "Mean", [src, b.cf(x.shape), b.node("Tanh", [src])])
    if pick in ("reduce_l2", "reduce_log_sum_exp", "reduce_max") and x.ndim >= 2 and x.size >= 16:
        op = {"reduce_l2": "ReduceL2", "reduce_log_sum_exp": "ReduceLogSumExp", "reduce_max": "ReduceMax"}[pick]
        b.opset = 18  # the axes of these three are an input from opset 18 on
        return b.node(op, [src, b.ci([int(r.integers(x.ndim))])], keepdims=1)
    if pick == "global_max_pool" and four:
        return b.node("GlobalMaxPool", [src])
    if pick == "cum_sum" and x.ndim >= 1:
        return b.node("CumSum", [src, b.const(np.array(int(r.integers(x.ndim)), np.int64), "i")])
    if pick == "trilu" and x.ndim >= 2:
        return b.node("Trilu", [src, b.const(np.array(int(r.integers(-1, 2)), np.int64), "i")], upper=int(r.integers(2)))
    if pick == "tile" and x.ndim >= 1 and x.size * 2 <= MAX_ELEMS:
        reps = [1] * x.ndim
        reps[int(r.integers(x.ndim))] = 2
        return b.node("Tile", [src, b.ci(reps)])
    if pick == "gather_elements" and x.ndim >= 1:
        ax = int(r.integers(x.ndim))
        return b.node("GatherElements", [src, b.const(r.integers(0, x.shape[ax], x.shape).astype(np.int64), "i")], axis=ax)
    if pick == "depth_to_space" and four and x.shape[1] % 4 == 0:
        return b.node("DepthToSpace", [src], blocksize=2, mode="DCR")
    if pick == "resize_nearest" and four and small:
        return b.node("Resize", [src, "", b.const(np.array([1.0, 1.0, 2.0, 2.0], F))], mode="nearest")
    return None


def _link(b, src, prev):
    """`src` shifted by the mean of `prev` (ReduceMean over every axis, broadcasting Sub): the next motif's operand depends on the previous result."""
    mean = b.node("ReduceMean", [prev], axes=list(range(b.v[prev].ndim)), keepdims=1)
    return b.node("Sub", [src, b.node("Reshape", [mean, b.ci([1])])])


def hand_case(row):
    """The minimal graph of one table row: an input, the motif, its results as outputs."""
    if row == "shape/dynamic_batch_reshape":
        return shape_case()
    motif, variant = row.split("/", 1)
    b = Builder("hand_" + row.replace("/", "_"), seed=1 + ROWS.index(row))
    src = b.inp((4, 96))
    for o in MOTIFS[motif][0](b, variant, src):
        b.out(o)
    return b.finish()


def shape_case():
    """Shape -> Gather -> Unsqueeze -> Concat -> Reshape around a Conv + Relu, with the leading axis dynamic and bound at 2 and at 3."""
    b = Builder("hand_shape_dynamic_batch_reshape", seed=977)
    x = b.inp((2, 3, 6, 6), dims=["batch", 3, 6, 6])
    y = b.node("Relu", [b.node("Conv", [x, b.cf((4, 3, 3, 3), 0.4), b.cf((4,))], kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[1, 1])])
    shp = b.node("Shape", [y])
    n = b.node("Gather", [shp, b.const(np.array(0, np.int64), "i")], axis=0)
    n1 = b.node("Unsqueeze", [n, b.ci([0])])
    tgt = b.node("Concat", [n1, b.ci([-1])], axis=0)
    flat = b.node("Reshape", [y, tgt])
    z = b.node("Add", [b.node("MatMul", [flat, b.cf((4 * 36, 10), 0.2)]), b.cf((10,))])
    b.out(z)
    b.out(flat)
    b.row("shape/dynamic_batch_reshape", 2, ["Conv+Relu", "FusedMatMul"])
    b.case.expect["modes_differ"] = "FusedMatMul bias position"
    b.alt = {x: Builder("alt", 978).data((3, 3, 6, 6))}
    return b.finish()


def make_case(seed):
    """A random graph of 6-30 nodes: the one or two table rows the seed stands for plus motifs drawn at random, each reading the graph input shifted by
    the previous motif's result, with glue in between and behind; deterministic from the seed alone."""
    new = seed >= OLD_SEEDS
    if new:  # the extended table: the rows added after the first corpus, by stride, among motifs drawn from the whole table
        forced = [NEW_ROWS[k].split("/", 1) for k in range(seed - OLD_SEEDS, len(NEW_ROWS), N_SEEDS - OLD_SEEDS)]
    else:
        motif_rows = OLD_ROWS[:-len(HAND_ONLY_ROWS)]
        forced = [motif_rows[k].split("/", 1) for k in range(seed % OLD_SEEDS, len(motif_rows), OLD_SEEDS)]  # every row occurs in the random corpus too
    motifs = MOTIFS if new else OLD_MOTIFS
    for attempt in range(64):
        b = Builder(f"seed{seed}", seed=(seed << 8) + attempt)
        b.later_k = 7 * seed + attempt
        r = b.rng
        src = b.inp((int(r.integers(6, 10)), 320))
        picks = [forced[k] for k in r.permutation(len(forced))]
        prev, results = None, []
        while picks or (len(b.case.nodes) < 14 and r.integers(3)):
            motif, variant = picks.pop(0) if picks else (str(r.choice(list(motifs))), None)
            fn, variants = motifs[motif]
            variant = variant or str(r.choice([v for v in variants if v not in ("bias_len_mismatch", "v_head_count_differs")]))  # an expected error ends the run: only where the seed asks
            cur = src if prev is None else _link(b, src, prev)
            if len(b.case.nodes) < 12 and r.integers(2):
                cur = (glue_later if new and r.integers(2) else glue)(b, cur)
            outs = fn(b, variant, cur)
            results += outs
            prev = next((o for o in outs if b.v[o].dtype == F), prev)
        for o in results:
            if b.v[o].dtype == F and len(b.case.nodes) < (MAX_NODES_NEW - 6 if new else 27) and r.integers(2):
                o = (glue_later if new and r.integers(2) else glue)(b, o)
            if o not in b.case.outputs:
                b.out(o)
        if 6 <= len(b.case.nodes) <= (MAX_NODES_NEW if new else 30):
            return b.finish()
    raise AssertionError(f"seed {seed}: no graph of the allowed size in 64 attempts")


def corpus():
    """Every case of the committed corpus: one hand-written graph per table row, then the random seeds."""
    return [hand_case(r) for r in ROWS] + [make_case(s) for s in range(N_SEEDS)]


PROBE = os.path.join(ROOT, "tests", "cpp", "_build", "graph_outputs_outlive_run")


def build_outlive_probe():
    """tests/cpp/graph_outputs_outlive_run.cpp: runs a graph, reuses the pool, THEN reads the outputs (the CLI reads them first)."""
    import subprocess
    from rten_amd import lib as L
    L.load()
    src = os.path.join(ROOT, "tests", "cpp", "graph_outputs_outlive_run.cpp")
    deps = [src] + [os.path.join(ROOT, "include", h) for h in ("rten_hip_graph.hpp", "rten_hip_ops.hpp", "rten_hip_safetensors.hpp", "rten_hip.h")]
    os.makedirs(os.path.dirname(PROBE), exist_ok=True)
    if not os.path.exists(PROBE) or os.path.getmtime(PROBE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", PROBE,
                               "-L" + os.path.join(ROOT, "rten_amd"), "-lrten_hip", "-Wl,-rpath,$ORIGIN/../../../rten_amd",
                               "-Wl,-rpath," + os.path.join(ROOT, "rten_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return PROBE
