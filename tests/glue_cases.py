"""One table of glue-operator cases for every evaluator: the g++ host program (tests/test_glue_ops.py), the product path with device operands and
with host operands, the path-flip pairs, the fusion modes and the raw kernels (tests/test_gpu_glue.py).

A case is (operator, attributes, operands, expected).  The expected value ALWAYS comes from tests/glue_rules.py, never from the code under test.

Operands are placed by `place`:
  "data"   the operand the mode moves: a graph input in the device mode, an initializer in the host mode
  "init"   always an initializer (shape operands the executor must know on the host; a CONSTANT divisor)
  "input"  always a graph input (a RUN-TIME divisor, run-time indices)
`want_host` / `want_dev` are the expected results of the two modes: an array, ("error", kind, message), or None when the mode does not apply
(a rank-7 case has no host mode: host values share the 6-dim broadcast helper; NonZero and Range have no device mode beyond their refusal).
"""
import functools

import numpy as np

from rten_amd import onnx_writer as ow
from tests import glue_rules as R
from tests.math_rules import RuleError

F, I32, I64, U8, I8 = np.float32, np.int32, np.int64, np.uint8, np.int8
GRID_CAP = 2048 * 256  # ew_blocks (rten_amd/csrc/elementwise.hip): at most 2048 workgroups of 256 lanes; one more element is a second grid-stride trip
PAST_CAP = GRID_CAP + 5
HOST_CONST = 4096      # Graph::upload: an initializer of at most this many elements carries a host value
I32_MIN, I32_MAX = R.I32_MIN, R.I32_MAX
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
NAN_PAYLOAD = np.array([0x7FA00001], np.uint32).view(F)[0]
HOST_PROGRAM_OPS = {"Shape", "Add", "Sub", "Mul", "Div", "And", "Or", "Xor", "Equal", "Less", "LessOrEqual", "Greater", "GreaterOrEqual", "Not", "Where", "Cast",
                    "Transpose", "Gather", "Concat", "Slice", "Expand", "ConstantOfShape", "NonZero", "Range", "Flatten", "Reshape", "Squeeze", "Unsqueeze"}
COMPARISONS = ("Equal", "Less", "LessOrEqual", "Greater", "GreaterOrEqual")
RANK7 = "more than 6 dims"


class Case:
    def __init__(self, cid, op, inputs, place, want_host, want_dev, attrs=None, value=None, pair=None):
        self.id, self.op, self.inputs, self.place = cid, op, inputs, place
        self.want_host, self.want_dev, self.attrs, self.value, self.pair = want_host, want_dev, attrs or {}, value, pair

    def __repr__(self):
        return self.id

    @property
    def host_program(self):
        """Evaluated by tests/cpp/test_glue_hostops.cpp: every operand could carry a host value (float32 / int32 / int64)."""
        return (self.want_host is not None and self.op in HOST_PROGRAM_OPS and "input" not in self.place
                and all(a is None or (a.dtype in (F, I32, I64) and a.size <= 2 * HOST_CONST) for a in self.inputs))

    @property
    def hosted(self):
        """The product evaluates the host mode of this case on the host: every operand is a small float32 / integer initializer."""
        return self.host_program and all(a is None or a.size <= HOST_CONST for a in self.inputs) and not (self.op == "Cast" and self.attrs["to"] in (ow.UINT8, ow.INT8))


def ruled(fn):
    """The rules' result, or ("error", kind, message)."""
    try:
        with np.errstate(all="ignore"):
            return np.array(fn(), order="C")  # (ascontiguousarray would turn a 0-d result into shape [1])
    except RuleError as e:
        return ("error", e.kind, e.msg)


def refusal(msg):
    return ("error", "UnsupportedValue", msg)


def _f(rng, shape, lo=-2.0, hi=2.0):
    return rng.uniform(lo, hi, shape).astype(F)


def _i(rng, shape, lo=-50, hi=50):
    return rng.integers(lo, hi, shape).astype(I32)


# ------------------------------------------------------------------------------------------------ shapes every broadcasting operator is swept over
EQUAL_SHAPES = [(), (1,), (5,), (255,), (256,), (257,), (2, 3, 1, 2, 3, 2), (3, 0, 4)]
BROADCAST_PAIRS = [
    ((1, 3, 4), (2, 3, 4)), ((2, 1, 4), (2, 3, 4)), ((2, 3, 1), (2, 3, 4)),      # the left operand broadcast on a leading, middle, trailing axis
    ((2, 3, 4), (1, 3, 4)), ((2, 3, 4), (2, 1, 4)), ((2, 3, 4), (2, 3, 1)),      # the right operand
    ((2, 1, 4), (1, 3, 1)), ((3, 1), (1, 4)),                                    # both
    ((2, 3, 4), ()), ((2, 3, 4), (1,)), ((2, 3, 4), (1, 1, 1)),                  # a one-element operand at ranks 0, 1, 3
    ((), (2, 3, 4)), ((1,), (2, 3, 4)), ((1, 1, 1), (2, 3, 4)),
    ((2, 3, 1, 2, 1, 2), (1, 3, 2, 1, 3, 2)),                                    # rank 6, both
    ((3, 0, 4), (4,)), ((3, 1, 4), (1, 0, 1)),                                   # a zero-size dimension: OK, nothing written
    ((4,), (2, 3, 4)), ((2, 3, 4), (3, 4)),                                      # ranks differ
]
SHORT_PAIRS = [((5,), (5,)), ((2, 1, 4), (1, 3, 1)), ((2, 3, 4), ()), ((), (2, 3, 4))]
RANK7_PAIR = ((2, 1, 2, 1, 2, 1, 2), (1, 2, 1, 2, 1, 2, 1))


def _binary(out, tag, op, rule, make, pairs, dev_rule=None):
    for sa, sb in pairs:
        a, b = make(sa), make(sb)
        want = ruled(lambda: rule(a, b))
        dev = want if dev_rule is None else ruled(lambda: dev_rule(a, b))
        out.append(Case(f"{tag}-{_s(sa)}-{_s(sb)}", op, [a, b], ["data", "data"], want, dev))


def _s(shape):
    return "x".join(str(d) for d in shape) or "scalar"


@functools.lru_cache(maxsize=None)
def table():
    rng = np.random.default_rng(20240611)
    out = []
    all_pairs = [(s, s) for s in EQUAL_SHAPES] + BROADCAST_PAIRS

    # ---- float32 Add / Sub / Mul / Div: the flat kernels (equal shapes, trailing blocks) and binary_bcast_kernel
    fl = lambda s: _f(rng, s, 0.5, 3.0) * rng.choice(np.array([-1, 1], F), s)
    _binary(out, "add-f32", "Add", lambda a, b: R.farith("Add", a, b), fl, all_pairs)
    _binary(out, "div-f32", "Div", R.div_f32, fl, all_pairs)
    for op in ("Sub", "Mul"):
        _binary(out, f"{op.lower()}-f32", op, lambda a, b, op=op: R.farith(op, a, b), fl, SHORT_PAIRS)
    # ---- int32 Add / Sub / Mul / Div (generic_nd_kernel): a constant divisor is checked on the host, a run-time one gives 0 per zero element
    it = lambda s: _i(rng, s)
    nz = lambda s: np.where(_i(rng, s) == 0, 3, _i(rng, s, 1, 9)).astype(I32)
    _binary(out, "add-i32", "Add", lambda a, b: R.iarith("Add", a, b), it, all_pairs)
    for op in ("Sub", "Mul"):
        _binary(out, f"{op.lower()}-i32", op, lambda a, b, op=op: R.iarith(op, a, b), it, SHORT_PAIRS)
    for sa, sb in SHORT_PAIRS + [((3, 0, 4), (4,))]:
        a, b = it(sa), nz(sb)
        out.append(Case(f"div-i32-{_s(sa)}-{_s(sb)}", "Div", [a, b], ["data", "data"], ruled(lambda: R.idiv(a, b)), ruled(lambda: R.idiv_device(a, b))))
    # ---- logic and comparisons
    bl = lambda s: rng.choice(np.array([0, 1, -3, I32_MIN], I32), s)
    _binary(out, "and", "And", lambda a, b: R.logical("And", a, b), bl, all_pairs)
    for op in ("Or", "Xor"):
        _binary(out, op.lower(), op, lambda a, b, op=op: R.logical(op, a, b), bl, SHORT_PAIRS)
    fc = lambda s: rng.choice(np.array([0.0, -0.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 2.0], F), s)
    ic = lambda s: rng.choice(np.array([I32_MIN, I32_MAX, -1, 0, 1, 7], I32), s)
    _binary(out, "equal-f32", "Equal", lambda a, b: R.compare("Equal", a, b), fc, all_pairs)
    for op in COMPARISONS:
        _binary(out, f"{op.lower()}-f32", op, lambda a, b, op=op: R.compare(op, a, b), fc, SHORT_PAIRS if op != "Equal" else [])
        _binary(out, f"{op.lower()}-i32", op, lambda a, b, op=op: R.compare(op, a, b), ic, SHORT_PAIRS)
    # NaN on either side, +0 against -0: every comparison
    sa = np.array([np.nan, 1.0, np.nan, 0.0, -0.0, NAN_PAYLOAD, np.inf, -np.inf], F)
    sb = np.array([1.0, np.nan, np.nan, -0.0, 0.0, NAN_PAYLOAD, np.inf, np.inf], F)
    for op in COMPARISONS:
        out.append(Case(f"{op.lower()}-f32-specials", op, [sa, sb], ["data", "data"], *[ruled(lambda: R.compare(op, sa, sb))] * 2))
    for s in EQUAL_SHAPES:
        x = bl(s)
        out.append(Case(f"not-{_s(s)}", "Not", [x], ["data"], *[ruled(lambda: R.logical_not(x))] * 2))
    # ---- Where: three-way broadcasts; float payloads must survive as bits
    payload = lambda s: rng.choice(np.array([0x7FA00001, 0xFFC12345, 0x80000000, 0x00000001, 0x7F800000, 0x3F800000], np.uint32), s).view(F).reshape(s)
    for sc, sx, sy in [((), (), ()), ((5,), (5,), (5,)), ((257,), (257,), ()), ((2, 3, 1, 2, 3, 2),) * 3, ((3, 0, 4), (3, 0, 4), (4,)), ((2, 1, 4), (1, 3, 1), (4,)),
                       ((1,), (2, 3, 4), (1, 1, 1)), ((2, 3, 4), (), (3, 1)), ((2, 3, 1, 2, 1, 2), (1, 3, 2, 1, 3, 2), (2,))]:
        c, x, y = bl(sc), payload(sx), payload(sy)
        out.append(Case(f"where-f32-{_s(sc)}-{_s(sx)}-{_s(sy)}", "Where", [c, x, y], ["data"] * 3, *[ruled(lambda: R.where(c, x, y))] * 2))
    c, x, y = bl((2, 1, 4)), ic((1, 3, 1)), ic((4,))
    out.append(Case("where-i32-bcast", "Where", [c, x, y], ["data"] * 3, *[ruled(lambda: R.where(c, x, y))] * 2))

    # ---- rank 7: refused by every operator of the N-d kernels (the flat kernels -- Cast, Not, equal-shape float arithmetic, Concat, Gather -- have no rank limit)
    r7a, r7b = RANK7_PAIR
    out.append(Case("rank7-add-f32", "Add", [fl(r7a), fl(r7b)], ["data"] * 2, None, refusal(RANK7)))
    out.append(Case("rank7-add-i32", "Add", [it(r7a), it(r7b)], ["data"] * 2, None, refusal(RANK7)))
    out.append(Case("rank7-and", "And", [bl(r7a), bl(r7b)], ["data"] * 2, None, refusal(RANK7)))
    out.append(Case("rank7-equal", "Equal", [fc(r7a), fc(r7b)], ["data"] * 2, None, refusal(RANK7)))
    out.append(Case("rank7-where", "Where", [bl(r7a), fl(r7b), fl(())], ["data"] * 3, None, refusal(RANK7)))
    out.append(Case("rank7-transpose", "Transpose", [fl(r7a)], ["data"], None, ("error", "InvalidValue", "at most 6 dims")))
    out.append(Case("rank7-slice", "Slice", [fl(r7a), np.array([0], I64), np.array([1], I64), np.array([0], I64)], ["data", "init", "init", "init"], None, refusal(RANK7)))
    out.append(Case("rank7-expand", "Expand", [fl(r7a), np.array(r7b, I64)], ["data", "init"], None, refusal(RANK7)))

    # ---- just past the grid cap: the second trip of every device kernel's grid-stride loop (device mode only: nothing this large is a host value)
    n = PAST_CAP
    big_f, big_i = _f(rng, (n,)), _i(rng, (n,), -1000, 1000)
    one_f, one_i = np.array([1.25], F), np.array(7, I32)
    dev_only = lambda cid, op, ins, place, want, **kw: out.append(Case(cid, op, ins, place, None, want, **kw))
    dev_only("cap-add-i32", "Add", [big_i, one_i], ["data", "data"], ruled(lambda: R.iarith("Add", big_i, one_i)))                               # generic_nd_kernel
    dev_only("cap-add-f32-bcast", "Add", [big_f, big_f.reshape(1, n)], ["data", "data"], ruled(lambda: R.farith("Add", big_f, big_f.reshape(1, n))))  # binary_bcast_kernel
    dev_only("cap-cast-f32-i32", "Cast", [big_f * 1000], ["data"], ruled(lambda: R.cast(big_f * 1000, I32)), attrs={"to": ow.INT32})
    dev_only("cap-transpose", "Transpose", [big_f.reshape(n, 1)], ["data"], ruled(lambda: R.transpose(big_f.reshape(n, 1))))                      # permute_kernel
    dev_only("cap-expand", "Expand", [one_f, np.array([n], I64)], ["data", "init"], ruled(lambda: R.expand(one_f, [n])))                          # permute_kernel, stride 0
    dev_only("cap-slice-reverse", "Slice", [big_f, np.array([-1], I64), np.array([I64_MIN + 1], I64), np.array([0], I64), np.array([-1], I64)],
             ["data"] + ["init"] * 4, ruled(lambda: R.slice(big_f, [-1], [I64_MIN + 1], [0], [-1])))                                             # generic_nd_kernel, signed strides
    ids = rng.integers(-6, 6, (n,)).astype(I32)
    tab_i, tab_f = _i(rng, (6,)), _f(rng, (6, 1))
    dev_only("cap-gather-axis", "Gather", [tab_i, ids], ["data", "data"], ruled(lambda: R.gather(tab_i, ids, 0)), attrs={"axis": 0})             # gather_axis_kernel
    dev_only("cap-gather-rows", "Gather", [tab_f, ids], ["data", "data"], ruled(lambda: R.gather(tab_f, ids, 0)), attrs={"axis": 0})             # gather_rows_kernel
    dev_only("cap-concat", "Concat", [big_f, one_f], ["data", "data"], ruled(lambda: R.concat([big_f, one_f], 0)), attrs={"axis": 0})            # copy_rows_kernel

    # ---- the same node on the two paths: an initializer of exactly 4096 elements is a host value, one of 4097 is not
    def pair(tag, op, make, rule, attrs=None, place=None):
        for m in (HOST_CONST, HOST_CONST + 1):
            ins = make(m)
            want = ruled(lambda: rule(*ins))
            out.append(Case(f"flip-{tag}-{m}", op, ins, place or ["data"] * len(ins), want, want, attrs=attrs, pair=tag))
    base_f, base_i = _f(rng, (HOST_CONST + 1,)), _i(rng, (HOST_CONST + 1,))
    base_g = _f(rng, (HOST_CONST + 1,), 0.5, 2.0)
    pair("add-f32", "Add", lambda m: [base_f[:m], base_g[:m]], lambda a, b: R.farith("Add", a, b))
    pair("div-f32-by-3", "Div", lambda m: [base_f[:m], np.array(3.0, F)], R.div_f32)
    pair("div-f32", "Div", lambda m: [base_f[:m], base_g[:m]], R.div_f32)
    pair("mul-i32", "Mul", lambda m: [base_i[:m] * 60000, base_i[:m] * 37 + 1], lambda a, b: R.iarith("Mul", a, b))
    pair("div-i32", "Div", lambda m: [base_i[:m], np.array(-7, I32)], R.idiv)
    pair("sub-f32", "Sub", lambda m: [base_f[:m], base_g[:m]], lambda a, b: R.farith("Sub", a, b))
    pair("and", "And", lambda m: [base_i[:m] % 2, base_i[:m] % 5], lambda a, b: R.logical("And", a, b))
    pair("equal-i32", "Equal", lambda m: [base_i[:m] % 4, base_i[:m] % 3], lambda a, b: R.compare("Equal", a, b))
    pair("reshape", "Reshape", lambda m: [base_f[:m], np.array([1, -1], I64)], lambda x, t: R.reshape(x, t), place=["data", "init"])
    pair("xor", "Xor", lambda m: [base_i[:m] % 2, base_i[:m] % 3], lambda a, b: R.logical("Xor", a, b))
    pair("less-f32", "Less", lambda m: [base_f[:m], base_g[:m] - 1], lambda a, b: R.compare("Less", a, b))
    pair("not", "Not", lambda m: [base_i[:m] % 2], R.logical_not)
    pair("where", "Where", lambda m: [base_i[:m] % 2, base_f[:m], np.array(-0.0, F)], R.where)
    pair("cast-f32-i32", "Cast", lambda m: [base_f[:m] * 100], lambda x: R.cast(x, I32), attrs={"to": ow.INT32})
    pair("cast-i32-f32", "Cast", lambda m: [base_i[:m] * 400000], lambda x: R.cast(x, F), attrs={"to": ow.FLOAT})
    pair("transpose", "Transpose", lambda m: [base_f[:m].reshape(m // 17, 17) if m % 17 == 0 else base_f[:m].reshape(m // 64, 64) if m % 64 == 0 else base_f[:m].reshape(m, 1)],
         R.transpose)
    pair("gather", "Gather", lambda m: [base_i[:m], np.array([[0, -1], [m - 1, -m]], I32)], lambda x, i: R.gather(x, i, 0), attrs={"axis": 0})
    pair("concat", "Concat", lambda m: [base_f[:m], np.array([1.0, 2.0, 3.0], F)], lambda a, b: R.concat([a, b], 0), attrs={"axis": 0})
    pair("slice-reverse", "Slice", lambda m: [base_f[:m], np.array([-1], I64), np.array([I64_MIN], I64), np.array([0], I64), np.array([-3], I64)],
         lambda x, s, e, a, st: R.slice(x, s, e, a, st), place=["data", "init", "init", "init", "init"])
    pair("expand", "Expand", lambda m: [base_f[:m], np.array([2, 1], I64)], R.expand, place=["data", "init"])

    # ---- Slice
    spec = np.array([0.0, -0.0, 1.0, NAN_PAYLOAD, -2.5, np.inf, 7.0], F)
    sl = lambda cid, x, starts, ends, axes=None, steps=None: out.append(Case(
        cid, "Slice", [x, np.array(starts, I64), np.array(ends, I64)] + ([np.array(axes, I64)] if axes is not None or steps is not None else []) +
        ([np.array(steps, I64)] if steps is not None else []), ["data"] + ["init"] * (2 + (axes is not None or steps is not None) + (steps is not None)),
        *[ruled(lambda: R.slice(x, starts, ends, axes, steps))] * 2))
    for step in (1, 2, 3, -1, -2, -3):
        fwd = step > 0
        sl(f"slice-step{step}-all", spec, [0 if fwd else -1], [I64_MAX if fwd else I64_MIN + 1], [0], [step])
        sl(f"slice-step{step}-inner", spec, [1 if fwd else 5], [6 if fwd else 0], [0], [step])
        sl(f"slice-step{step}-beyond", spec, [-100 if fwd else 100], [100 if fwd else -100], [0], [step])
        sl(f"slice-step{step}-negative-bounds", spec, [-6 if fwd else -2], [-1 if fwd else -7], [0], [step])
        sl(f"slice-step{step}-empty", spec, [4 if fwd else 2], [4 if fwd else 2], [0], [step])
        sl(f"slice-step{step}-empty-crossed", spec, [5 if fwd else 1], [2 if fwd else 4], [0], [step])
    sl("slice-int64-extremes", spec, [I64_MIN + 1], [I64_MAX], [0], [1])
    sl("slice-int64-min-end-backward", spec, [I64_MAX], [I64_MIN], [0], [-1])
    m57 = _f(rng, (5, 7))
    sl("slice-two-axes", m57, [1, 2], [4, 6], [0, 1], [1, 2])
    sl("slice-axes-out-of-order", m57, [6, 0], [0, 5], [1, 0], [-2, 3])
    sl("slice-negative-axes", m57, [1, -3], [I64_MAX, I64_MIN + 1], [-1, -2], [1, -1])
    sl("slice-no-axes", m57, [1, 2], [4, 6])
    sl("slice-both-reversed", m57, [-1, -1], [I64_MIN, I64_MIN], [0, 1], [-1, -1])
    r6 = _i(rng, (2, 3, 1, 2, 3, 2))
    sl("slice-rank6", r6, [1, 2, 0], [3, 0, 2], [1, 4, 5], [1, -1, 2])
    sl("slice-rank1-of-1", np.array([4.0], F), [0], [1], [0], [1])
    sl("slice-zero-size", _f(rng, (3, 0, 4)), [1], [3], [0], [1])
    sl("slice-zero-size-backward", _f(rng, (3, 0, 4)), [-1], [I64_MIN], [1], [-1])
    sl("slice-257", _f(rng, (257,)), [256], [I64_MIN], [0], [-1])
    sl("slice-error-step-zero", spec, [0], [3], [0], [0])
    sl("slice-error-starts-length", m57, [0, 0, 0], [1, 1], [0, 1], [1, 1])
    sl("slice-error-ends-length", m57, [0, 0], [1], [0, 1], [1, 1])
    sl("slice-error-steps-length", m57, [0, 0], [1, 1], [0, 1], [1])
    sl("slice-error-axes-length", m57, [0, 0, 0], [1, 1, 1], [0, 1, 0], [1, 1, 1])
    sl("slice-error-axis", m57, [0], [1], [2], [1])
    for cid, x, st, en, ax in [("slice-attrs", m57, [1, -4], [3, 100], [0, 1]), ("slice-attrs-no-axes", m57, [2, 1], [I64_MAX, 3], None), ("slice-attrs-empty", spec, [5], [2], [0])]:
        attrs = {"starts": st, "ends": en, **({"axes": ax} if ax is not None else {})}
        out.append(Case(cid, "Slice", [x], ["data"], *[ruled(lambda: R.slice_attrs(x, st, en, ax))] * 2, attrs=attrs))

    # ---- integer values
    sv = np.array([I32_MIN, I32_MAX, -1, 0, 1, 7, -7, 2], I32)
    sw = np.array([-1, I32_MAX, I32_MIN, I32_MIN, I32_MAX, -3, 3, I32_MAX], I32)
    for op in ("Add", "Sub", "Mul"):
        out.append(Case(f"{op.lower()}-i32-wraps", op, [sv, sw], ["data"] * 2, *[ruled(lambda: R.iarith(op, sv, sw))] * 2))
    out.append(Case("div-i32-negative-truncates", "Div", [np.array([-7, 7, -7, 7, -1, I32_MIN, I32_MAX, I32_MIN], I32), np.array([2, -2, -2, 2, 2, 2, -1, I32_MIN], I32)], ["data"] * 2,
                    *[ruled(lambda: R.idiv([-7, 7, -7, 7, -1, I32_MIN, I32_MAX, I32_MIN], [2, -2, -2, 2, 2, 2, -1, I32_MIN]))] * 2))
    out.append(Case("div-i32-min-by-minus-one", "Div", [sv, np.array(-1, I32)], ["data"] * 2, *[ruled(lambda: R.idiv(sv, -1))] * 2))  # pinned: i32::MIN (Rust panics)
    zd = np.array([1, 0, 1, 1], I32)
    out.append(Case("div-i32-by-zero-constant", "Div", [np.array([1, 2, 3, 4], I32), zd], ["data", "init"], *[ruled(lambda: R.idiv([1, 2, 3, 4], zd))] * 2))
    out.append(Case("div-i32-by-zero-constant-empty-dividend", "Div", [np.zeros((0, 4), I32), zd], ["data", "init"], *[ruled(lambda: R.idiv(np.zeros((0, 4), I32), zd))] * 2))
    out.append(Case("div-i32-by-zero-run-time", "Div", [sv, sw * np.array([1, 0, 1, 0, 1, 1, 0, 1], I32)], ["data", "input"],
                    *[ruled(lambda: R.idiv_device(sv, sw * np.array([1, 0, 1, 0, 1, 1, 0, 1], I32)))] * 2))

    # ---- Cast: Rust `as`
    def cast(cid, x, to):
        code = {F: ow.FLOAT, I32: ow.INT32, U8: ow.UINT8, I8: ow.INT8}[to]
        out.append(Case(cid, "Cast", [x], ["data"], *[ruled(lambda: R.cast(x, to))] * 2, attrs={"to": code}))
    cast("cast-i32-f32-edges", np.array([(1 << 24) + 1, (1 << 24) + 3, I32_MAX, I32_MIN, -(1 << 24) - 1, 0, -1, I32_MAX - 64], I32), F)
    cast("cast-f32-i32-edges", np.array([2147483520.0, 2147483648.0, -2147483648.0, 3e10, -3e10, np.nan, 0.9, -0.9, -0.0, np.inf, -np.inf, 1.5, -1.5, NAN_PAYLOAD], F), I32)
    cast("cast-f32-u8-edges", np.array([255.0, 255.5, 256.0, -0.9, np.nan, -1.0, 0.5, 254.9, 1e9, -np.inf], F), U8)
    cast("cast-f32-i8-edges", np.array([127.9, -128.9, -129.0, 127.0, 128.0, -128.0, np.nan, -0.9, 0.9, np.inf], F), I8)
    cast("cast-i32-u8-wraps", np.array([0, 255, 256, -1, 511, I32_MIN, I32_MAX, -129], I32), U8)
    cast("cast-i32-i8-wraps", np.array([0, 127, 128, -128, -129, 255, I32_MIN, I32_MAX], I32), I8)
    codes_u, codes_i = np.arange(256, dtype=U8), np.arange(256, dtype=U8).view(I8)
    cast("cast-u8-i8-all-codes", codes_u, I8)
    cast("cast-i8-u8-all-codes", codes_i, U8)
    cast("cast-i8-f32-all-codes", codes_i, F)
    cast("cast-u8-i32-all-codes", codes_u, I32)
    cast("cast-u8-f32-all-codes", codes_u, F)
    cast("cast-i8-i32-all-codes", codes_i, I32)
    for s in [(), (1,), (257,), (2, 3, 1, 2, 3, 2), (3, 0, 4)]:
        cast(f"cast-f32-i32-{_s(s)}", _f(rng, s, -300, 300), I32)
    cast("cast-f32-f32-copy", spec, F)
    cast("cast-i32-i32-copy", sv, I32)

    # ---- float Div: a divisor of ONE element, at any rank, multiplies by the reciprocal; anything else divides
    xs = np.concatenate([_f(rng, (61,), -9, 9), np.array([0.0, -0.0, np.inf, np.nan, 1e-38, 3e38], F)])
    for d in (3.0, 1.4142135, 0.1, 8.0, 0.0):
        for s in ((), (1,), (1, 1, 1)):
            dv = np.full(s, d, F)
            for where, place in (("init", ["data", "init"]), ("input", ["data", "input"])):
                out.append(Case(f"div-f32-by-{d}-{_s(s)}-{where}", "Div", [xs, dv], place, *[ruled(lambda: R.div_f32(xs, dv))] * 2))
            out.append(Case(f"div-f32-{d}-{_s(s)}-on-the-left", "Div", [dv, xs], ["data", "data"], *[ruled(lambda: R.div_f32(dv, xs))] * 2))
    two = np.array([3.0, 0.1], F)
    out.append(Case("div-f32-by-two-elements", "Div", [xs[:66].reshape(33, 2), two], ["data", "init"], *[ruled(lambda: R.div_f32(xs[:66].reshape(33, 2), two))] * 2))
    out.append(Case("div-f32-one-by-one", "Div", [np.array([7.0], F), np.array(3.0, F)], ["data", "data"], *[ruled(lambda: R.div_f32([7.0], 3.0))] * 2))

    # ---- Range, ConstantOfShape, NonZero: host values only (the output's SHAPE depends on the operands' values)
    host_only = lambda cid, op, ins, want, **kw: out.append(Case(cid, op, ins, ["init"] * len(ins), want, None, **kw))
    for cid, (a, b, d) in {"range-f32-tenths": (0.0, 1.0, 0.1), "range-f32-seven-tenths": (0.0, 0.7, 0.1), "range-f32-negative-delta": (2.0, -1.0, -0.3), "range-f32-empty": (1.0, 0.0, 0.5),
                           "range-f32-delta-zero": (0.0, 1.0, 0.0), "range-f32-thirds": (-1.0, 1.0, 1.0 / 3), "range-f32-257": (0.0, 25.7, 0.1)}.items():
        host_only(cid, "Range", [np.array(v, F) for v in (a, b, d)], ruled(lambda: R.range_(F(a), F(b), F(d))))
    for cid, (a, b, d) in {"range-i32-end-not-hit": (-5, 6, 3), "range-i32-negative-delta": (10, 3, -2), "range-i32-empty": (3, 3, 1), "range-i32-delta-zero": (0, 5, 0),
                           "range-i32-256": (0, 256, 1), "range-i64-operands": (0, 5, 2)}.items():
        dt = I64 if "i64" in cid else I32
        host_only(cid, "Range", [np.array(v, dt) for v in (a, b, d)], ruled(lambda: R.range_(I32(a), I32(b), I32(d))))
    out.append(Case("range-of-run-time-operands", "Range", [np.array([0.0], F), np.array([1.0], F), np.array([0.5], F)], ["input"] * 3, None,
                    refusal("Range: start / limit / delta must be constants or computable from the input shapes")))
    for cid, shape_values, value in [("constant-default", [2, 3], None), ("constant-f32", [4], np.array([-0.0], F)), ("constant-f32-nan-payload", [3], np.array([NAN_PAYLOAD], F)),
                                     ("constant-i32", [1, 5, 2], np.array([42], I32)), ("constant-i32-min", [2], np.array([I32_MIN], I32)), ("constant-i64", [3], np.array([-5], I64)),
                                     ("constant-i64-max", [2, 2], np.array([I64_MAX], I64)), ("constant-i64-min", [2], np.array([I64_MIN], I64)),
                                     ("constant-i64-above-i32", [1], np.array([1 << 32], I64)), ("constant-negative-dim", [1, -1], np.array([42], I32)),
                                     ("constant-zero-dim", [3, 0, 4], np.array([1.5], F)), ("constant-scalar", [], np.array([2.5], F)), ("constant-257", [257], np.array([7], I64)),
                                     ("constant-rank6", [2, 3, 1, 2, 3, 2], None)]:
        host_only(cid, "ConstantOfShape", [np.array(shape_values, I64)], ruled(lambda: R.constant_of_shape(shape_values, None if value is None else value[0])), value=value)
    for cid, x in {"nonzero-rank1": np.array([0, 3, 0, -1, 0], I32), "nonzero-rank2": np.array([[0.0, 1.0], [1.0, 1.0]], F), "nonzero-rank3": _i(rng, (2, 3, 4), 0, 2),
                   "nonzero-all-zero": np.zeros((2, 3), I32), "nonzero-none-zero": np.ones((3, 2), I32), "nonzero-f32-signed-zero-and-nan": np.array([-0.0, 0.0, np.nan, NAN_PAYLOAD, 1e-45, -1.0], F),
                   "nonzero-scalar": np.array(3.0, F), "nonzero-scalar-zero": np.array(0, I32), "nonzero-empty": np.zeros((3, 0, 4), F), "nonzero-257": (np.arange(257) % 3).astype(I32)}.items():
        host_only(cid, "NonZero", [x], ruled(lambda: R.nonzero(x)))
    out.append(Case("nonzero-of-run-time-data", "NonZero", [np.array([0.0, 1.0], F)], ["input"], None, refusal("NonZero of device data")))

    # ---- Expand
    ex = lambda cid, x, target: out.append(Case(cid, "Expand", [x, np.array(target, I64)], ["data", "init"], *[ruled(lambda: R.expand(x, target))] * 2))
    ex("expand-scalar", np.array(5, I32), [2, 2])
    ex("expand-rank0-to-rank0", np.array(1.5, F), [])
    ex("expand-rank-grows", _i(rng, (3, 1)), [2, 3, 1])
    ex("expand-both-contribute", _i(rng, (3, 1)), [2, 1, 6])
    ex("expand-leading-and-trailing", _f(rng, (1, 2, 1)), [2, 2, 2])
    ex("expand-middle", _f(rng, (2, 1, 2)), [2, 2, 2])
    ex("expand-target-of-ones", _f(rng, (2, 3)), [1, 1])
    ex("expand-rank6", _f(rng, (2, 1, 1, 2, 1, 2)), [1, 3, 2, 1, 3, 1])
    ex("expand-zero-size", _f(rng, (3, 1, 4)), [3, 0, 4])
    ex("expand-257", _f(rng, (1,)), [257])
    ex("expand-error-shapes", np.array([1, 2, 3], I32), [2, 2])
    ex("expand-error-negative", np.array([1], I32), [-1])

    # ---- Gather
    g3 = _f(rng, (3, 4, 5))
    gi = _i(rng, (3, 4, 5))
    ga = lambda cid, x, ids, axis, dev=None, place=None: out.append(Case(cid, "Gather", [x, ids], place or ["data", "data"], ruled(lambda: R.gather(x, ids, axis)),
                                                                      ruled(lambda: (dev or R.gather)(x, ids, axis)), attrs={"axis": axis}))
    for axis in (0, 1, 2, -1, -3):
        n_ax = g3.shape[axis]
        ga(f"gather-f32-axis{axis}-2d-ids", g3, np.array([[0, n_ax - 1], [-1, -n_ax]], I32), axis)
        ga(f"gather-i32-axis{axis}-scalar-id", gi, np.array(-2, I32), axis)
    ga("gather-vector-scalar-id", np.array([4, 5, 6], I32), np.array(1, I32), 0)
    ga("gather-257", _f(rng, (257, 3)), np.array([256, -257, 0, 255], I32), 0)
    ga("gather-rank6", _f(rng, (2, 3, 1, 2, 3, 2)), np.array([2, 0], I32), 4)
    ga("gather-empty-ids", np.array([1, 2, 3], I32), np.zeros((0,), I32), 0)
    ga("gather-zero-size-inner", _f(rng, (3, 0, 4)), np.array([2, 0], I32), 0)
    ga("gather-out-of-range", gi, np.array([[2, 5], [-4, 3]], I32), 0, dev=R.gather_device)            # host: the reference's error; device: clamped
    ga("gather-out-of-range-f32-rows", g3, np.array([3, -7, 100, I32_MIN, I32_MAX], I32), 0, dev=R.gather_device)
    ga("gather-out-of-range-axis1", g3, np.array([4, -5], I32), 1, dev=R.gather_device)
    ga("gather-error-axis", g3, np.array([0], I32), 3)

    # ---- Concat
    ca = lambda cid, xs, axis: out.append(Case(cid, "Concat", xs, ["data"] * len(xs), *[ruled(lambda: R.concat(xs, axis))] * 2, attrs={"axis": axis}))
    a221, b221 = _f(rng, (2, 2, 1)), _f(rng, (2, 2, 1))
    ca("concat-one-input", [a221], 0)
    ca("concat-first-axis", [a221, b221], 0)
    ca("concat-last-axis", [a221, b221], 2)
    ca("concat-negative-axis", [a221, b221, a221], -2)
    ca("concat-three-inputs", [_i(rng, (2, 3)), _i(rng, (2, 1)), _i(rng, (2, 257))], 1)
    ca("concat-empty-piece", [np.array([1, 2, 3], I32), np.zeros((0,), I32), np.array([4, 5, 6], I32)], 0)
    ca("concat-rank6", [_f(rng, (2, 3, 1, 2, 3, 2)), _f(rng, (2, 3, 1, 5, 3, 2))], 3)
    ca("concat-zero-size", [_f(rng, (3, 0, 4)), _f(rng, (3, 0, 4))], 0)
    ca("concat-error-rank", [np.zeros((1,), F), np.zeros((1, 2), F)], 0)
    ca("concat-error-extent", [np.zeros((5, 10), F), np.zeros((5, 11), F)], 0)
    ca("concat-error-axis", [np.array([1, 2, 3], I32), np.array([1, 2, 3], I32)], 1)

    # ---- Transpose, Shape and the views
    tr = lambda cid, x, perm: out.append(Case(cid, "Transpose", [x], ["data"], *[ruled(lambda: R.transpose(x, perm))] * 2, attrs={} if perm is None else {"perm": list(perm)}))
    tr("transpose-default", g3, None)
    tr("transpose-rank0", np.array(2.0, F), None)
    tr("transpose-rank1", _f(rng, (257,)), None)
    tr("transpose-negative-perm", gi, (-1, 0, 1))
    tr("transpose-rank6", _f(rng, (2, 3, 1, 2, 3, 2)), (5, 3, 4, 0, 2, 1))
    tr("transpose-zero-size", _f(rng, (3, 0, 4)), (2, 0, 1))
    tr("transpose-256x3", _f(rng, (256, 3)), (1, 0))
    tr("transpose-error-repeated", g3, (0, 1, 1))
    tr("transpose-error-length", g3, (0, 1))
    for cid, s, start, end in [("shape-all", (2, 3, 4), None, None), ("shape-start", (2, 3, 4), 1, None), ("shape-negative", (2, 3, 4), -2, -1), ("shape-clamped", (2, 3, 4), -9, 9),
                               ("shape-crossed", (2, 3, 4), 2, 1), ("shape-rank0", (), None, None), ("shape-zero-size", (3, 0, 4), 0, 2), ("shape-rank6", (2, 3, 1, 2, 3, 2), 1, -1)]:
        attrs = {**({"start": start} if start is not None else {}), **({"end": end} if end is not None else {})}
        out.append(Case(cid, "Shape", [np.zeros(s, F)], ["data"], *[ruled(lambda: R.shape(s, start, end))] * 2, attrs=attrs))
    vw = lambda cid, op, x, spec_values, rule, **attrs: out.append(Case(cid, op, [x] + ([np.array(spec_values, I64)] if spec_values is not None else []),
                                                                     ["data"] + (["init"] if spec_values is not None else []), *[ruled(rule)] * 2, attrs=attrs))
    v6 = _f(rng, (2, 1, 3, 1))
    vw("squeeze-all", "Squeeze", v6, None, lambda: R.squeeze(v6))
    vw("squeeze-axes", "Squeeze", v6, [-1], lambda: R.squeeze(v6, [-1]))
    vw("squeeze-error", "Squeeze", v6, [0], lambda: R.squeeze(v6, [0]))
    vw("unsqueeze", "Unsqueeze", gi, [0, -1], lambda: R.unsqueeze(gi, [0, -1]))
    vw("unsqueeze-rank0", "Unsqueeze", np.array(3, I32), [0], lambda: R.unsqueeze(np.array(3, I32), [0]))
    vw("reshape-infer", "Reshape", g3, [0, -1], lambda: R.reshape(g3, [0, -1]))
    vw("reshape-to-scalar", "Reshape", np.array([[4.0]], F), [], lambda: R.reshape(np.array([[4.0]], F), []))
    vw("reshape-zero-size", "Reshape", _f(rng, (3, 0, 4)), [0, 0, 2, 2], lambda: R.reshape(np.zeros((3, 0, 4), F), [0, 0, 2, 2]))
    vw("reshape-allowzero", "Reshape", _f(rng, (0, 0, 10)), [10, 0, 0], lambda: R.reshape(np.zeros((0, 0, 10), F), [10, 0, 0], True), allowzero=1)
    z8 = _i(rng, (2, 8))
    for cid, x, target in [("reshape-error-length", z8, [9]), ("reshape-error-multiple-of-product", z8, [1, 8]), ("reshape-error-zero-without-dim", z8, [2, 8, 0]),
                           ("reshape-error-two-inferred", z8, [-1, -1]), ("reshape-error-infer-beside-zero", _f(rng, (0, 4)), [0, -1]), ("reshape-error-below-minus-one", z8, [-2, 8]),
                           ("reshape-error-infer-not-a-divisor", z8, [3, -1])]:
        vw(cid, "Reshape", x, target, lambda: R.reshape(x, target))
    vw("squeeze-error-axis", "Squeeze", v6, [4], lambda: R.squeeze(v6, [4]))
    vw("unsqueeze-error-axis", "Unsqueeze", z8, [3], lambda: R.unsqueeze(z8, [3]))
    vw("unsqueeze-error-repeated", "Unsqueeze", z8, [1, -3], lambda: R.unsqueeze(z8, [1, -3]))
    vw("flatten-error-axis", "Flatten", g3, None, lambda: R.flatten(g3, 4), axis=4)
    vw("flatten-rank0", "Flatten", np.array(2.0, F), None, lambda: R.flatten(np.array(2.0, F), 0), axis=0)
    vw("flatten-default", "Flatten", g3, None, lambda: R.flatten(g3))
    vw("flatten-axis-rank", "Flatten", g3, None, lambda: R.flatten(g3, 3), axis=3)
    vw("flatten-negative-axis", "Flatten", g3, None, lambda: R.flatten(g3, -1), axis=-1)

    ids_seen = set()
    for c in out:
        assert c.id not in ids_seen, c.id
        ids_seen.add(c.id)
    return tuple(out)


def by_id(cid):
    return next(c for c in table() if c.id == cid)


# One case per operator for the fusion-mode runs (unfused, fused, captured and replayed)
FUSION_SUBSET = ["add-f32-2x1x4-1x3x1", "div-f32-by-3.0-scalar-init", "div-f32-by-3.0-1-input", "sub-f32-2x3x4-scalar", "mul-i32-2x1x4-1x3x1", "div-i32-5-5", "and-2x1x4-1x3x1",
                 "xor-5-5", "equal-f32-2x1x4-1x3x1", "less-i32-5-5", "not-5", "where-f32-2x1x4-1x3x1-4", "cast-f32-i32-257", "slice-axes-out-of-order", "slice-attrs",
                 "expand-both-contribute", "gather-f32-axis1-2d-ids", "concat-three-inputs", "transpose-negative-perm", "shape-negative", "squeeze-axes", "unsqueeze",
                 "reshape-infer", "flatten-default", "range-f32-tenths", "constant-i64-max", "nonzero-rank2"]
