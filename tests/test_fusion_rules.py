"""tests/fusion_rules.py pinned: spellings with the answer the reference's matcher and optimiser give by their rules, each with its cite.  The rows
marked (ref test) restate the cases of the reference's own tests (src/optimize/pattern_matcher.rs:587-852, src/optimize/tests.rs) on this file's
graphs; the others follow from the cited lines."""
import collections
import json
import os

import numpy as np

from tests import fusion_rules as fr

F = np.float32
SQRT2 = np.sqrt(F(2.0))


class G:
    """A tiny graph builder: values are names, constants are one-element float32 arrays unless given."""

    def __init__(self):
        self.nodes, self.consts, self.k = [], {}, 0

    def c(self, value, shape=()):
        self.k += 1
        name = f"c{self.k}"
        self.consts[name] = np.asarray(value).astype(F).reshape(shape) if not isinstance(value, np.ndarray) else value
        return name

    def __call__(self, op, *inputs, **attrs):
        self.k += 1
        out = f"{op.lower()}{self.k}"
        self.nodes.append({"op": op, "inputs": list(inputs), "outputs": [out], "attrs": attrs, "name": "n_" + out})
        return out

    def ops(self, outputs, ranks=None):
        nodes, _, log = fr.rewrite(self.nodes, self.consts, outputs, {"x": 3, "y": 3} if ranks is None else ranks)
        return sorted(collections.Counter(n["op"] for n in nodes).items()), nodes, log


def erf_plus_1(g, x="x", sqrt2=SQRT2, inner="div", one=1.0):
    s = g("Div", x, g.c(sqrt2)) if inner == "div" else g("Mul", x, g.c(F(1.0) / F(sqrt2)))
    return g("Add", g("Erf", s), g.c(one))


def gelu(form, x="x", half=0.5, **kw):
    g = G()
    e, h = erf_plus_1(g, x, **kw), g.c(half)
    out = {"(x*e)*h": lambda: g("Mul", g("Mul", x, e), h), "h*(x*e)": lambda: g("Mul", h, g("Mul", x, e)), "(x*h)*e": lambda: g("Mul", g("Mul", x, h), e),
           "x*(e*h)": lambda: g("Mul", x, g("Mul", e, h)), "x*(h*e)": lambda: g("Mul", x, g("Mul", h, e)), "(e*x)*h": lambda: g("Mul", g("Mul", e, x), h)}[form]()
    return g, out


GELU, FIVE = [("Gelu", 1)], [("Add", 1), ("Div", 1), ("Erf", 1), ("Mul", 2)]


def test_gelu_bracketings_and_tolerance():
    for form in ("(x*e)*h", "h*(x*e)", "(x*h)*e", "x*(e*h)", "x*(h*e)", "(e*x)*h"):  # (ref test) tests.rs:535-564; pattern_matcher.rs:159-169
        g, out = gelu(form)
        assert g.ops([out])[0] == GELU, form
    g, out = gelu("(x*e)*h", inner="mul")  # fusions.rs:419: any_of [x / sqrt2, x * (1 / sqrt2)]
    assert g.ops([out])[0] == GELU
    # CONST_TOLERANCE is absolute 1e-4 (pattern_matcher.rs:91-92, :115-122)
    for half, want in ((0.5 + 9e-5, True), (0.5 - 9e-5, True), (0.5 + 2e-4, False), (0.5 - 2e-4, False), (0.50001, True)):
        g, out = gelu("(x*e)*h", half=half)
        assert (g.ops([out])[0] == GELU) == want, half
    g, out = gelu("(x*e)*h", sqrt2=1.4142)
    assert g.ops([out])[0] == GELU
    g, out = gelu("(x*e)*h", sqrt2=1.4144)  # 1.86e-4 away
    assert g.ops([out])[0] == FIVE
    g, out = gelu("(x*e)*h", one=1.00001)  # (ref test) pattern_matcher.rs:642-648
    assert g.ops([out])[0] == GELU
    g, out = gelu("(x*e)*h", one=1.1)  # (ref test) pattern_matcher.rs:636-641
    assert g.ops([out])[0] == FIVE


def test_gelu_constant_forms():
    for shape, want in (((), True), ((1,), True), ((1, 1), True)):  # TensorView::item: one element at any rank (rten-tensor/src/tensor.rs:1821-1830)
        g = G()
        e = g("Add", g("Erf", g("Div", "x", g.c(SQRT2, shape))), g.c(1.0, shape))
        out = g("Mul", g("Mul", "x", e), g.c(0.5, shape))
        assert (g.ops([out])[0] == GELU) == want, shape
    g = G()  # two elements: item() is None
    e = erf_plus_1(g)
    out = g("Mul", g("Mul", "x", e), g.c(np.array([0.5, 0.5], F)))
    assert g.ops([out])[0] == FIVE
    g = G()  # an integer constant is no float constant (pattern_matcher.rs:116-121)
    e = erf_plus_1(g)
    g.consts["half"] = np.array(1, np.int32)
    out = g("Mul", g("Mul", "x", e), "half")
    assert g.ops([out])[0] == FIVE


def test_gelu_spoilers():
    g, out = gelu("(x*e)*h")  # (ref test) tests.rs:1139-1159: the Erf output read by another operator
    erf = [n for n in g.nodes if n["op"] == "Erf"][0]["outputs"][0]
    neg = g("Neg", erf)
    assert g.ops([out, neg])[0] == FIVE + [("Neg", 1)]
    g, out = gelu("(x*e)*h")  # (ref test) tests.rs:1193-1216: the Erf output is a graph output
    assert g.ops([out, erf])[0] == FIVE
    g, out = gelu("(x*e)*h")  # the inner product is a graph output
    inner = g.nodes[-1]["inputs"][0]
    assert g.ops([out, inner])[0] == FIVE
    g = G()  # x differs between the two uses: the symbol binds once (pattern_matcher.rs:497-504; (ref test) :649-655)
    out = g("Mul", g("Mul", "x", erf_plus_1(g, "y")), g.c(0.5))
    assert g.ops([out])[0] == FIVE
    g = G()  # 0.5 replaced by a value
    out = g("Mul", g("Mul", "x", erf_plus_1(g)), "y")
    assert g.ops([out])[0] == FIVE
    # x itself a product: the graph chain has 4 operands, the pattern's 3 (pattern_matcher.rs:163), so the strict commutative rule decides: the
    # pattern's own bracketing (either operand order) fuses, the others do not
    for form, want in (("(x*e)*h", True), ("h*(x*e)", True), ("(e*x)*h", True), ("(x*h)*e", False), ("x*(e*h)", False), ("x*(h*e)", False)):
        g = G()
        p = g("Mul", "x", "y")
        e, h = erf_plus_1(g, p), g.c(0.5)
        out = {"(x*e)*h": lambda: g("Mul", g("Mul", p, e), h), "h*(x*e)": lambda: g("Mul", h, g("Mul", p, e)), "(e*x)*h": lambda: g("Mul", g("Mul", e, p), h),
               "(x*h)*e": lambda: g("Mul", g("Mul", p, h), e), "x*(e*h)": lambda: g("Mul", p, g("Mul", e, h)), "x*(h*e)": lambda: g("Mul", p, g("Mul", h, e))}[form]()
        got = g.ops([out])[0]
        assert (got == [("Gelu", 1), ("Mul", 1)]) == want, (form, got)
        assert want or got == [("Add", 1), ("Div", 1), ("Erf", 1), ("Mul", 3)], (form, got)


def test_matcher_rules():
    x, y, z, w = (fr.sym(s) for s in "xyzw")
    view = lambda g: fr.View(g.nodes, g.consts, [], {})
    root = lambda g: len(g.nodes) - 1
    # (ref test) pattern_matcher.rs:587-663 on softsign x / (1 + |x|)
    g = G()
    g("Div", "x", g("Add", g.c(1.0), g("Abs", "x")))
    c = fr.const_sym("c")
    for pat, want in ((fr.op("Div", x, fr.op("Add", 1.0, fr.op("Abs", x))), True), (fr.op("Div", x, fr.op("Add", c, fr.op("Abs", x))), True),
                      (fr.op("Div", fr.op("Add", 1.0, fr.op("Abs", x)), x), False),   # operands of "/" swapped
                      (fr.op("Div", x, fr.op("Add", fr.op("Abs", x), 1.0)), True),    # operands of "+" swapped
                      (fr.op("Div", x, fr.op("Sub", 1.0, fr.op("Abs", x))), False), (fr.op("Div", x, fr.op("Add", 1.1, fr.op("Abs", x))), False),
                      (fr.op("Div", x, fr.op("Add", 1.00001, fr.op("Abs", x))), True), (fr.op("Div", x, fr.op("Add", x, fr.op("Abs", x))), False),
                      (fr.op("Div", c, fr.op("Add", 1.0, fr.op("Abs", x))), False)):  # a value against a const symbol
        m = fr.match_at(pat, root(g), view(g))
        assert (m is not None) == want
        assert m is None or m["x"] == "x"
    m = fr.match_at(fr.op("Div", x, fr.op("Add", 1.0, fr.op("Abs", x, key="abs_op"))), root(g), view(g))  # (ref test) :685-695
    assert g.nodes[m["abs_op"][1]]["op"] == "Abs"
    assert fr.match_at(fr.op("Div", x, fr.op("Add", fr.exact_const(1.00001), fr.op("Abs", x))), root(g), view(g)) is None  # exact_constant: tolerance 0 (:108-113)
    # (ref test) :731-776: (x * Pow(x, y)) * z against every bracketing and order, and against a chain of two
    pat = fr.op("Mul", fr.op("Mul", x, fr.op("Pow", x, y)), z)
    for build in (lambda g, a, p, c: g("Mul", g("Mul", a, p), c), lambda g, a, p, c: g("Mul", a, g("Mul", p, c)), lambda g, a, p, c: g("Mul", g("Mul", c, a), p),
                  lambda g, a, p, c: g("Mul", p, g("Mul", a, c))):
        g = G()
        build(g, "a", g("Pow", "a", "b"), "c")
        assert fr.match_at(pat, root(g), view(g)) is not None
    g = G()
    g("Mul", "a", g("Pow", "a", "b"))
    assert fr.match_at(pat, root(g), view(g)) is None
    # (ref test) :778-805: Equal is commutative, not associative: Equal(Equal(w, x), Equal(y, z)) does not match ((a == b) == c) == d
    g = G()
    g("Equal", g("Equal", g("Equal", "a", "b"), "c"), "d")
    assert fr.match_at(fr.op("Equal", fr.op("Equal", w, x), fr.op("Equal", y, z)), root(g), view(g)) is None
    # (ref test) :807-830: a keyed sub-pattern is not flattened, and its node is recorded
    g = G()
    g("Mul", g("Mul", "a", "b"), "c")
    m = fr.match_at(fr.op("Mul", fr.op("Mul", x, y, key="inner"), z), root(g), view(g))
    assert m is not None and g.nodes[m["inner"][1]]["op"] == "Mul" and m["inner"][1] == 0
    # (ref test) :832-852: x * y against a * b * c binds one symbol to the inner product
    m = fr.match_at(fr.op("Mul", x, y), root(g), view(g))
    assert m is not None and m["x"] != m["y"]


def silu(order, alpha=None, x2="x"):
    g = G()
    arg = "x" if alpha is None else (g("Mul", alpha(g), x2) if order[1] == "a" else g("Mul", x2, alpha(g)))
    s = g("Sigmoid", arg if alpha is not None else x2)
    return g, (g("Mul", "x", s) if order[0] == "x" else g("Mul", s, "x"))


def test_silu_and_swish():
    for order in ("x_", "s_"):  # (ref test) tests.rs:342-353; commutative: pattern_matcher.rs:171-187
        g, out = silu(order)
        assert g.ops([out])[0] == [("Silu", 1)]
    g, out = silu("x_", x2="y")  # Sigmoid of another value
    assert g.ops([out])[0] == [("Mul", 1), ("Sigmoid", 1)]
    g, out = silu("x_")  # the Sigmoid output read twice (optimize.rs:195-221)
    t = g("Neg", g.nodes[0]["outputs"][0])
    assert g.ops([out, t])[0] == [("Mul", 1), ("Neg", 1), ("Sigmoid", 1)]
    for order in ("xa", "xx", "sa", "sx"):  # (ref test) tests.rs:356-369, alpha 1.7, and the other operand orders
        for shape in ((), (1,)):
            g, out = silu(order, alpha=lambda g: g.c(1.7, shape))
            ops, nodes, _ = g.ops([out])
            assert ops == [("Swish", 1)] and nodes[0]["attrs"]["alpha"] == float(F(1.7)) and nodes[0]["inputs"] == ["x"]
    g, out = silu("xa", alpha=lambda g: g.c(np.array([1.0, 2.0, 3.0], F)))  # alpha not a scalar: "alpha not a scalar" (fusions.rs:609-614)
    assert g.ops([out])[0] == [("Mul", 2), ("Sigmoid", 1)]
    g, out = silu("xa", alpha=lambda g: "y")  # alpha a value: const_symbol (pattern_matcher.rs:493-495)
    assert g.ops([out])[0] == [("Mul", 2), ("Sigmoid", 1)]
    g, out = silu("xa", alpha=lambda g: g.c(1.7), x2="y")
    assert g.ops([out])[0] == [("Mul", 2), ("Sigmoid", 1)]


def layer_norm(g, x="x", x2=None, axes=(-1,), axes2=None, axes_input=False, keepdims=1, exponent=2.0, eps=1e-6, eps_first=False, scale=None, scale_first=False,
               bias=True, bias_first=False, eps_shape=()):
    mean = lambda v, ax: g("ReduceMean", v, g_axes(ax), keepdims=keepdims) if axes_input else g("ReduceMean", v, axes=list(ax), keepdims=keepdims)

    def g_axes(ax):
        g.k += 1
        g.consts[f"axes{g.k}"] = np.asarray(ax, np.int64)
        return f"axes{g.k}"
    center = g("Sub", x, mean(x2 or x, axes))
    var = mean(g("Pow", center, g.c(exponent)), axes2 or axes)
    e = g.c(eps, eps_shape)
    std = g("Sqrt", g("Add", e, var) if eps_first else g("Add", var, e))
    norm = g("Div", center, std)
    sc = scale or g.c(np.array([3., 4., 5.], F))
    y = g("Mul", sc, norm) if scale_first else g("Mul", norm, sc)
    if bias:
        bc = g.c(np.array([1., 2., 3.], F)) if bias is True else bias
        y = g("Add", bc, y) if bias_first else g("Add", y, bc)
    return y, center, var


LN = [("LayerNormalization", 1)]
LN_PARTS = [("Add", 1), ("Div", 1), ("Mul", 1), ("Pow", 1), ("ReduceMean", 2), ("Sqrt", 1), ("Sub", 1)]


def test_layer_norm():
    for kw in (dict(bias=True), dict(bias=False), dict(bias_first=True), dict(eps_first=True), dict(scale_first=True), dict(eps_shape=(1,)),
               dict(exponent=2.00005), dict(axes_input=True), dict(axes=(2,)), dict(axes=(2,), axes_input=True)):  # (ref test) tests.rs:603-644 are the first two
        g = G()
        y, _, _ = layer_norm(g, **kw)
        ops, nodes, log = g.ops([y])
        assert ops == LN, (kw, ops)
        n = nodes[0]
        assert n["attrs"] == {"axis": -1, "epsilon": float(F(1e-6))} and n["inputs"][0] == "x" and len(n["inputs"]) == (2 if kw.get("bias") is False else 3), kw
        assert n["outputs"] == [y]
        if kw.get("axes_input"):  # ReduceMeanAxesFusion in the first round, LayerNormalizationFusion in the second (optimize.rs:619-629, :652-659)
            assert [f for f, _ in log] == ["ReduceMeanAxesFusion"] * 2 + ["LayerNormalizationFusion"]
    plus_add = lambda parts: sorted(collections.Counter(dict(parts, Add=2)).items())
    for kw, why in ((dict(axes=(1,)), "an inner axis (fusions.rs:721-732)"), (dict(axes=(-1,), axes2=(1,)), "the variance over an inner axis"),
                    (dict(axes=(1, 2)), "two axes: get_axis is None (fusions.rs:627-633)"), (dict(exponent=3.0), "Pow exponent"),
                    (dict(exponent=2.0002), "Pow exponent outside the tolerance"), (dict(scale="y"), "scale is a value (const_symbol)"),
                    (dict(x2="y"), "the first mean over another input"), (dict(eps=np.array([1e-6, 1e-6, 1e-6], F)), "epsilon not a scalar (fusions.rs:734-737)")):
        g = G()
        if isinstance(kw.get("eps"), np.ndarray):
            arr = kw.pop("eps")
            y, _, _ = layer_norm(g, **kw)
            eps_name = [n for n in g.nodes if n["op"] == "Sqrt"][0]
            add = [n for n in g.nodes if n["outputs"][0] == eps_name["inputs"][0]][0]
            g.consts[add["inputs"][1]] = arr
        else:
            y, _, _ = layer_norm(g, **kw)
        assert g.ops([y])[0] == plus_add(LN_PARTS), why
    g = G()  # a positive last axis on a value of unknown rank (fusions.rs:660-670)
    y, _, _ = layer_norm(g, axes=(2,))
    assert g.ops([y], ranks={})[0] == plus_add(LN_PARTS)
    g = G()  # keepdims is not looked at (fusions.rs:716-743): a rank-1 input normalised with keepdims = 0 is the same function, and fuses
    y, _, _ = layer_norm(g, keepdims=0)
    assert g.ops([y], ranks={"x": 1})[0] == LN
    g = G()  # the centered value read a third time
    y, center, _ = layer_norm(g)
    t = g("Neg", center)
    assert g.ops([y, t])[0] == sorted(plus_add(LN_PARTS) + [("Neg", 1)])
    g = G()  # the variance a graph output
    y, _, var = layer_norm(g)
    assert g.ops([y, var])[0] == plus_add(LN_PARTS)
    g = G()  # bias is a value: the scale-only form fuses at the Mul, the Add stays (any_of, fusions.rs:706-709; reverse visit order, optimize.rs:142-149)
    y, _, _ = layer_norm(g, bias="y")
    ops, nodes, _ = g.ops([y])
    assert ops == [("Add", 1), ("LayerNormalization", 1)] and len([n for n in nodes if n["op"] == "LayerNormalization"][0]["inputs"]) == 2
    g = G()  # the scaled value read twice: the form with bias is dropped AFTER it has claimed its operators for the round (optimize.rs:186-221), so the
    y, _, _ = layer_norm(g)  # scale-only form is not tried at the Mul; the round applied nothing and the optimiser stops (optimize.rs:652-659)
    scaled = [n for n in g.nodes if n["op"] == "Mul"][0]["outputs"][0]
    t = g("Neg", scaled)
    ops, _, log = g.ops([y, t])
    assert ops == sorted(plus_add(LN_PARTS) + [("Neg", 1)]) and log == []


def test_rounds_and_order():
    g = G()  # Silu inside a Gelu's x: both fuse in one round, in reverse execution order
    s = g("Mul", "x", g("Sigmoid", "x"))
    out = g("Mul", g("Mul", s, erf_plus_1(g, s)), g.c(0.5))
    ops, _, log = g.ops([out])
    assert ops == [("Gelu", 1), ("Silu", 1)] and [f for f, _ in log] == ["GeluFusion", "SiluFusion"]
    g = G()  # Constant nodes are constants before anything is matched
    g.nodes.append({"op": "Constant", "inputs": [], "outputs": ["half"], "attrs": {"value": np.array(0.5, F)}, "name": "k"})
    out = g("Mul", g("Mul", "x", erf_plus_1(g)), "half")
    assert g.ops([out])[0] == GELU


def test_fusion_list_matches_the_doc_table():
    """docs/KERNELS.md lists every entry of the reference's fusion list with its status; tests/golden/reference_fusions.json is the same list."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    want = json.load(open(os.path.join(root, "tests", "golden", "reference_fusions.json")))
    doc = open(os.path.join(root, "docs", "KERNELS.md")).read().split("## Load-time rewrites and the reference's fusion list", 1)[1].split("\n## ", 1)[0]
    rows = [[c.strip().strip("`") for c in line.strip().strip("|").split("|")] for line in doc.splitlines() if line.startswith("| `")]
    assert [{"name": r[0], "status": r[1]} for r in rows] == want
    assert {e["status"] for e in want} == {"reproduced", "same bits by construction", "not reproduced"}
    restated = [f for f, _, _ in fr.FUSIONS]  # in the reference's list order, and every one of them reproduced
    assert [e["name"] for e in want if e["name"] in restated] == restated
    assert all(e["status"] == "reproduced" for e in want if e["name"] in restated)
