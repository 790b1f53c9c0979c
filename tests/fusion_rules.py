"""The reference's load-time idiom fusions, restated: its pattern matcher, the patterns of SiluFusion, SwishFusion, GeluFusion and
LayerNormalizationFusion (with ReduceMeanAxesFusion, which LayerNormalizationFusion relies on), and the rules under which its optimiser applies a
fusion.  CPU only; works on the node dicts of tests/graph_fuzz.py ({"op", "inputs", "outputs", "attrs", "name"}).

The matcher (src/optimize/pattern_matcher.rs):
  * an operator pattern matches a node of the same name and the same number of inputs (:139-145);
  * a commutative binary operator matches in either operand order (:171-187); every other operator input by input (:189-195);
  * an operator that is associative AND commutative (Add, Mul: src/ops/binary_elementwise.rs:512-518; Equal and its kin are commutative only, :571)
    matches as a multiset: the pattern chain is flattened through same-named two-input patterns that carry no key (:199-230), the graph chain
    through same-named two-input producers (:232-266), and if the pattern chain has >= 3 operands and both have equal lengths, any assignment of the
    patterns to distinct operands matches (:159-169, :268-315).  If that fails, or the pattern chain has 2 operands, the strict commutative rule
    still applies;
  * a symbol matches any constant or value, and the same node everywhere (:492-505); a const symbol matches constants only;
  * a float constant pattern matches a one-element float constant (any rank: rten-tensor/src/tensor.rs:1821-1830) within ABSOLUTE 1e-4
    (CONST_TOLERANCE, :91-92, :115-122); an exact constant with tolerance 0 (:108-113);
  * any_of tries its patterns from left to right (:506-516).

The application (src/optimize.rs:119-260, :611-660):
  * the operators are visited in REVERSE execution order (:142-149); per operator the first fusion of the list that returns a fusion wins
    (:770-787), in the list order ReduceMeanAxes, Silu, Swish, Gelu, LayerNormalization (:619-629);
  * the unfused subgraph is every operator between the fusion's inputs and the matched operator's outputs (:172-184).  A fusion that contains an
    operator an earlier fusion of this round has claimed is skipped -- and the operators it walked before finding that one stay claimed (:186-193);
  * a fusion whose interior values are read outside the subgraph, or are graph outputs, is dropped (:195-221, :437-477) -- AFTER its operators have
    been claimed for this round, so nothing inside it fuses in this round either;
  * rounds repeat until none applies, three at the most (:652-659).

What this file leaves out: the reference's other fusions (docs/KERNELS.md, "Load-time rewrites and the reference's fusion list"), which may claim
nodes in the same round.  `op_applied_to_last_axis` (src/optimize/fusions.rs:643-671) accepts a positive axis when the rank of the ReduceMean's
input is known; a graph input carries its declared shape from load (src/model/onnx_loader.rs:145-146, src/graph/node.rs:250-252) and shape
inference is on by default (src/model.rs:696), but whether an interior value has a rank depends on every operator before it: here `ranks` holds
the graph inputs' declared ranks, and `View.rank` carries a rank through the idiom's own operators only.
"""
import numpy as np

F = np.float32
CONST_TOLERANCE = F(1e-4)
COMMUTATIVE = ("Add", "Mul", "And", "Or", "Xor", "Equal")
ASSOCIATIVE = ("Add", "Mul")
RANK_BROADCAST = ("Add", "Sub", "Mul", "Div", "Pow")
MAX_ROUNDS = 3


# ------------------------------------------------------------------------------------------------ patterns
class Pat:
    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)


def op(name, *inputs, key=None):
    return Pat("op", name=name, inputs=[const(p) if isinstance(p, (int, float, np.floating)) else p for p in inputs], key=key)


def const(value, tolerance=CONST_TOLERANCE):
    return Pat("const", value=F(value), tolerance=F(tolerance))


def exact_const(value):
    return const(value, 0.0)


def sym(name):
    return Pat("sym", name=name, constant=False)


def const_sym(name):
    return Pat("sym", name=name, constant=True)


def any_of(*pats):
    return Pat("any", pats=list(pats))


# ------------------------------------------------------------------------------------------------ graph view
class View:
    """A node list with its constants: who makes and who reads every value."""

    def __init__(self, nodes, consts, outputs, ranks=None):
        self.nodes, self.consts, self.outputs = nodes, consts, list(outputs)
        self.ranks = dict(ranks or {})
        self.producer, self.consumers = {}, {}
        for i, n in enumerate(nodes):
            for o in n["outputs"]:
                if o:
                    self.producer[o] = i
            for s in n["inputs"]:
                if s:
                    self.consumers.setdefault(s, []).append(i)

    def rank(self, name):
        """The rank shape inference gives a value (module docstring): declared for a graph input, and carried through the operators of the
        idioms themselves -- broadcasting binary operators (src/ops/binary_elementwise.rs:534, :697, :949, :1120, :1184), Sqrt and ReduceMean
        (src/ops/reduce.rs:579); behind any other operator it is unknown here."""
        if not name:
            return None
        if name in self.consts:
            return np.asarray(self.consts[name]).ndim
        if name in self.ranks:
            return self.ranks[name]
        i = self.producer.get(name)
        if i is None:
            return None
        n = self.nodes[i]
        if n["op"] in RANK_BROADCAST and len(n["inputs"]) == 2:
            a, b = self.rank(n["inputs"][0]), self.rank(n["inputs"][1])
            return None if a is None or b is None else max(a, b)
        if n["op"] == "Sqrt":
            return self.rank(n["inputs"][0])
        if n["op"] == "ReduceMean":
            r = self.rank(n["inputs"][0])
            if r is None or int(n["attrs"].get("keepdims", 1)) == 1:
                return r
            axes = n["attrs"].get("axes")
            if axes is None and len(n["inputs"]) > 1 and n["inputs"][1] in self.consts:
                axes = np.asarray(self.consts[n["inputs"][1]]).ravel()
            return None if axes is None else r - len(axes)
        return None

    def scalar(self, name, kind="f"):
        """get_scalar: the single element of a constant of that element type, at any rank (src/graph/node.rs:468-470)."""
        a = self.consts.get(name)
        if a is None or np.asarray(a).size != 1 or np.asarray(a).dtype.kind != kind:
            return None
        return np.asarray(a).reshape(-1)[0]


def _flatten_pattern(p, name, out):
    if p.kind == "op" and p.name == name and len(p.inputs) == 2 and p.key is None:
        for q in p.inputs:
            _flatten_pattern(q, name, out)
    else:
        out.append(p)


def _flatten_graph(v, g, name, out):
    i = g.producer.get(v) if v not in g.consts else None
    if i is not None and g.nodes[i]["op"] == name and len(g.nodes[i]["inputs"]) == 2 and all(g.nodes[i]["inputs"]):
        for s in g.nodes[i]["inputs"]:
            _flatten_graph(s, g, name, out)
    else:
        out.append(v)


def _match_set(pats, vals, used, g, syms):
    if not pats:
        return True
    for i, v in enumerate(vals):
        if used[i]:
            continue
        mark = len(syms)
        if _test(pats[0], v, g, syms):
            used[i] = True
            if _match_set(pats[1:], vals, used, g, syms):
                return True
            used[i] = False
        del syms[mark:]
    return False


def _match_op(p, idx, g, syms):
    n = g.nodes[idx]
    if n["op"] != p.name or len(p.inputs) != len(n["inputs"]):
        return False
    if p.name in ASSOCIATIVE and p.name in COMMUTATIVE and len(p.inputs) == 2:
        pats = []
        for q in p.inputs:
            _flatten_pattern(q, p.name, pats)
        if len(pats) >= 3:
            vals = []
            if all(n["inputs"]):
                for s in n["inputs"]:
                    _flatten_graph(s, g, p.name, vals)
            if len(pats) == len(vals) and _match_set(pats, vals, [False] * len(vals), g, syms):
                return True
    if p.name in COMMUTATIVE and len(p.inputs) == 2 and all(n["inputs"]):
        a, b = n["inputs"]
        mark = len(syms)
        if _test(p.inputs[0], a, g, syms) and _test(p.inputs[1], b, g, syms):
            return True
        del syms[mark:]
        return _test(p.inputs[1], a, g, syms) and _test(p.inputs[0], b, g, syms)
    return all(s and _test(q, s, g, syms) for q, s in zip(p.inputs, n["inputs"]))


def _find(syms, name):
    for k, v in syms:
        if k == name:
            return v
    return None


def _test(p, v, g, syms):
    """Pattern against the VALUE `v` (a constant, a graph input or an operator's output)."""
    if p.kind == "any":
        for q in p.pats:
            mark = len(syms)
            if _test(q, v, g, syms):
                return True
            del syms[mark:]
        return False
    if p.kind == "op":
        if v in g.consts or v not in g.producer:
            return False
        if not _match_op(p, g.producer[v], g, syms):
            return False
        if p.key:
            syms.append((p.key, ("op", g.producer[v])))
        return True
    if p.kind == "const":
        a = g.consts.get(v)
        if a is None or np.asarray(a).dtype != F or np.asarray(a).size != 1:
            return False
        with np.errstate(all="ignore"):
            return bool(np.abs(F(np.asarray(a).reshape(-1)[0]) - p.value) <= p.tolerance)
    if p.constant and v not in g.consts:
        return False
    seen = _find(syms, p.name)
    if seen is None:
        syms.append((p.name, v))
        return True
    return seen == v


def match_at(p, idx, g):
    """Pattern against the operator node `idx` (Pattern::test on an operator id).  Returns {symbol or key: value name or ("op", index)} or None."""
    syms = []
    if p.kind == "any":
        for q in p.pats:
            del syms[:]
            if q.kind == "op" and _match_op(q, idx, g, syms):
                if q.key:
                    syms.append((q.key, ("op", idx)))
                break
        else:
            return None
    elif p.kind != "op" or not _match_op(p, idx, g, syms):
        return None
    elif p.key:
        syms.append((p.key, ("op", idx)))
    out = {}
    for k, v in syms:
        out.setdefault(k, v)
    return out


# ------------------------------------------------------------------------------------------------ the fusions
def _last_axis(g, opid):
    """op_applied_to_last_axis::<ReduceMean> (fusions.rs:643-671): one axis given as an attribute, -1 or the known rank - 1."""
    n = g.nodes[opid[1]]
    axes = n["attrs"].get("axes")
    if axes is None or len(axes) != 1:
        return False
    if int(axes[0]) == -1:
        return True
    rank = g.rank(n["inputs"][0]) if n["inputs"] and n["inputs"][0] else None
    return rank is not None and rank >= 1 and rank - 1 == int(axes[0])


def _silu():
    x = sym("x")
    return op("Mul", x, op("Sigmoid", x))  # fusions.rs:576-579


def _swish():
    x = sym("x")
    return op("Mul", x, op("Sigmoid", op("Mul", const_sym("alpha"), x)))  # fusions.rs:599-603


def _gelu():
    x = sym("x")
    sqrt2 = np.sqrt(F(2.0))
    x_scaled = any_of(op("Div", x, sqrt2), op("Mul", x, F(1.0) / sqrt2))  # fusions.rs:416-421
    return op("Mul", op("Mul", x, op("Add", op("Erf", x_scaled), 1.0)), 0.5)


def _layer_norm():
    x = sym("x")  # fusions.rs:683-710
    center = op("Sub", x, op("ReduceMean", x, key="center_mean"))
    normalized = op("Div", center, op("Sqrt", op("Add", const_sym("epsilon"), op("ReduceMean", op("Pow", center, 2.0), key="norm_mean"))))
    scaled = op("Mul", normalized, const_sym("scale"))
    return any_of(op("Add", scaled, const_sym("bias")), scaled)


def _fuse_mean_axes(m, g, root):
    axes = g.consts.get(m["axes"])  # get_vector::<i32>: a rank-1 integer constant (int64 is int32 from load on)
    if axes is None or np.asarray(axes).ndim != 1 or np.asarray(axes).dtype.kind != "i":
        return None
    return {"op": "ReduceMean", "inputs": [m["x"]], "attrs": {"axes": [int(a) for a in axes], "keepdims": int(root["attrs"].get("keepdims", 1))}}


def _fuse_swish(m, g, root):
    alpha = g.scalar(m["alpha"])
    return None if alpha is None else {"op": "Swish", "inputs": [m["x"]], "attrs": {"alpha": float(alpha)}}


def _fuse_layer_norm(m, g, root):
    if not _last_axis(g, m["norm_mean"]) or not _last_axis(g, m["center_mean"]):
        return None
    eps = g.scalar(m["epsilon"])
    if eps is None:
        return None
    return {"op": "LayerNormalization", "inputs": [m["x"], m["scale"]] + ([m["bias"]] if "bias" in m else []), "attrs": {"axis": -1, "epsilon": float(eps)}}


FUSIONS = [  # (name, pattern, the fused node or None when a check fails): src/optimize.rs:619-629
    ("ReduceMeanAxesFusion", op("ReduceMean", sym("x"), const_sym("axes"), key="mean"), _fuse_mean_axes),
    ("SiluFusion", _silu(), lambda m, g, root: {"op": "Silu", "inputs": [m["x"]], "attrs": {}}),
    ("SwishFusion", _swish(), _fuse_swish),
    ("GeluFusion", _gelu(), lambda m, g, root: {"op": "Gelu", "inputs": [m["x"]], "attrs": {}}),
    ("LayerNormalizationFusion", _layer_norm(), _fuse_layer_norm),
]


def _subgraph(g, root, inputs):
    """The operators between `inputs` and the node `root`, as Graph::execution_plan finds them: walking back from the root's operands."""
    seen, stack = [], [root]
    while stack:
        i = stack.pop()
        if i in seen:
            continue
        seen.append(i)
        for s in g.nodes[i]["inputs"]:
            if s and s not in inputs and s not in g.consts and s in g.producer:
                stack.append(g.producer[s])
    return sorted(seen)


def one_round(nodes, consts, outputs, ranks=None, fusions=FUSIONS):
    """(new node list, [(fusion name, root node name)]) after one visit of every operator."""
    g = View(nodes, consts, outputs, ranks)
    claimed, replace, applied = set(), {}, []
    for idx in reversed(range(len(nodes))):
        if idx in claimed:
            continue
        for name, pat, make in fusions:
            m = match_at(pat, idx, g)
            fused = make(m, g, nodes[idx]) if m is not None else None
            if fused is None:
                continue
            ops = _subgraph(g, idx, set(fused["inputs"]))
            clash = False
            for o in ops:  # (:186-193: claimed one by one, and left claimed if a later one clashes)
                if o in claimed:
                    clash = True
                    break
                claimed.add(o)
            if clash:
                break
            interior_read = False
            for o in ops:
                for v in nodes[o]["outputs"]:
                    if not v or v in nodes[idx]["outputs"]:
                        continue
                    if v in g.outputs or any(c not in ops for c in g.consumers.get(v, [])):
                        interior_read = True
            if interior_read:
                break
            fused.update(outputs=list(nodes[idx]["outputs"]), name=nodes[idx]["name"])
            replace[idx] = (fused, ops)
            applied.append((name, nodes[idx]["name"]))
            break
    gone = {o for _, ops in replace.values() for o in ops}
    out = []
    for i, n in enumerate(nodes):
        if i in replace:
            out.append(replace[i][0])
        elif i not in gone:
            out.append(n)
    return out, applied


def fold_constant_dequantize(nodes, consts, outputs):
    """Constant propagation (src/optimize.rs:598-605) as far as the loader reproduces it: a DequantizeLinear whose operands are all constants becomes a
    float32 constant (tests/qdq_rules.py gives its value), unless its result is a graph output; an operand no node reads any more is dropped.  The
    reference folds EVERY operator over constants; the others give the same bits whether they run at load or per run, so nothing else is restated."""
    from tests import qdq_rules as QR
    kept, log, operands = [], [], set()
    for n in nodes:
        ins = [s for s in n["inputs"] if s]
        if n["op"] == "DequantizeLinear" and len(ins) >= 2 and all(s in consts for s in ins) and n["outputs"][0] not in outputs:
            consts[n["outputs"][0]] = QR.dequantize_linear(consts[ins[0]], consts[ins[1]], consts[ins[2]] if len(ins) > 2 else None, axis=n["attrs"].get("axis", 1))
            operands.update(ins)
            log.append(("ConstantPropagation", n["name"]))
        else:
            kept.append(n)
    for name in operands:
        if name not in outputs and not any(name in n["inputs"] for n in kept):
            del consts[name]
    return kept, log


def rewrite(nodes, consts, outputs, ranks=None):
    """The node list as the reference runs it, as far as these fusions go: (nodes, constants, [(fusion, root)]).  `Constant` nodes become
    constants first (the loader makes them constant nodes: src/model/onnx_loader.rs)."""
    consts = dict(consts)
    kept = []
    for n in nodes:
        if n["op"] == "Constant":
            consts[n["outputs"][0]] = np.asarray(n["attrs"]["value"])
        else:
            kept.append(n)
    nodes, log = fold_constant_dequantize(kept, consts, outputs)
    for _ in range(MAX_ROUNDS):
        nodes, applied = one_round(nodes, consts, outputs, ranks)
        log += applied
        if not applied:
            break
    return nodes, consts, log
