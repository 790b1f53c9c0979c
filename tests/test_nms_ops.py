"""NonMaxSuppression without a device: the rule (tests/nms_rules.py) against the reference's own literals (tests/golden/nms_reference.json); the named
cases that tell the reference's rule from textbook score-sorted per-class NMS; the Python host operator on a recording context (argument marshalling,
every error); header, ctypes table and Rust bindings; and what `rten_hip_run --parse-only` prints for, and refuses about, the detector head graph."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import nms_cases as NC  # noqa: E402
from tests import nms_rules as R  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "nms_reference.json")))
F, I = np.float32, np.int32
SYMBOL = "rten_hip_non_max_suppression_f32"


def example_boxes(order):
    """gen_boxes_scores (non_max_suppression.rs:253-280) on the golden file's example_boxes."""
    ex = GOLDEN["example_boxes"]
    boxes = np.array([[b["tlbr"] for b in ex]], F)
    scores = np.zeros((1, max(b["class"] for b in ex) + 1, len(ex)), F)
    for i, b in enumerate(ex):
        scores[0, b["class"], i] = b["score"]
    return (NC.to_center(boxes) if order == "cwh" else boxes), scores


# ---------------------------------------------------------------------------------------------- 1. the rule
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_rule_reproduces_the_reference_literals(case):
    boxes, scores = example_boxes(case["box_order"])
    rows = R.non_max_suppression(boxes, scores, 0, case["max_output_boxes_per_class"], case["iou_threshold"], case["score_threshold"])
    assert rows.dtype == I and rows.shape == (case["rows"], 3)
    for i, want in case["asserted_rows"].items():
        assert rows[int(i)].tolist() == want


def test_rule_box_orders_errors_and_no_classes():
    case = GOLDEN["box_order_case"]
    tlbr, scores = example_boxes("tlbr")
    cwh, _ = example_boxes("cwh")
    a = R.non_max_suppression(tlbr, scores, 0, None, case["iou_threshold"], case["score_threshold"])
    b = R.non_max_suppression(cwh, scores, 1, None, case["iou_threshold"], case["score_threshold"])
    assert len(a) == 3 and np.array_equal(a, b)
    for bad in GOLDEN["invalid"]:
        with pytest.raises(R.RuleError) as e:
            R.non_max_suppression(np.zeros(bad["boxes_shape"], F), np.zeros(bad["scores_shape"], F), 0, None, 0.5, 0.0)
        assert [e.value.kind, e.value.msg] == bad["error"]
    nc = GOLDEN["no_classes"]
    assert R.non_max_suppression(np.zeros(nc["boxes_shape"], F), np.zeros(nc["scores_shape"], F)).shape == tuple(nc["rows_shape"])


def test_total_order_and_narrowing():
    neg_nan = np.array([0xFFC00000], np.uint32).view(F)[0]
    order = [neg_nan, -np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf, np.nan]
    keys = [R.total_key(F(v)) for v in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert R.saturate_i32(2 ** 63 - 1) == 2 ** 31 - 1 and R.saturate_i32(-2 ** 63) == -2 ** 31 and R.saturate_i32(7) == 7
    assert np.isnan(R.iou((F(5), F(5), F(5), F(5)), (F(5), F(5), F(5), F(5))))         # 0 / 0
    assert R.iou((F(0), F(0), F(10), F(10)), (F(np.nan), F(0), F(10), F(10))) == F(1)  # min / max ignore the NaN


NAMED = NC.named_cases()


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_cases_tell_the_rule_from_textbook_nms(name):
    case = NAMED[name]
    rows = R.non_max_suppression(case["boxes"], case["scores"], **case["kw"])
    canon = lambda r: sorted(map(tuple, np.asarray(r).tolist()))
    if case["differs_from_textbook"]:
        assert canon(rows) != canon(NC.textbook(case["boxes"], case["scores"], **case["kw"])), name
    # the [cx, cy, w, h] form of the same boxes gives the same rows (halves and sums of these small integers are exact)
    if np.isfinite(case["boxes"]).all():
        assert np.array_equal(R.non_max_suppression(NC.to_center(case["boxes"]), case["scores"], 1, **case["kw"]), rows)
    want = {"removed_by_a_rejected_candidate": [[0, 0, 1]], "cross_image_suppression": [[0, 0, 0]], "cross_image_replacement": [[1, 0, 0]],
            "cross_class_suppression": [[0, 0, 0]], "cap_counted_across_images": [[1, 0, 0]], "hull_versus_union": [[0, 0, 0], [0, 0, 1]],
            "ties_in_score": [[0, 0, 1], [1, 0, 0], [1, 0, 2], [0, 0, 0], [0, 0, 2], [1, 0, 1]], "class_ties_last_wins": [[0, 2, 2], [0, 2, 1], [0, 2, 0]],
            "signed_zero_class_scores": [[0, 0, 0], [0, 1, 1], [0, 1, 3], [0, 1, 2]], "nan_scores": [[0, 0, 0], [0, 0, 2]],
            "nan_coordinates": [[0, 0, 3], [0, 0, 1]], "degenerate_boxes": [[0, 0, 3]], "degenerate_only": [[0, 0, 1], [0, 0, 0], [0, 0, 2]],
            "negative_cap": [], "zero_cap": [], "cap_of_two": [[0, 0, 1], [0, 0, 3], [0, 1, 0], [0, 1, 2]]}
    if name in want:  # worked out by hand from non_max_suppression.rs
        assert rows.tolist() == want[name], name
    if name in ("absent_cap", "saturated_cap"):
        assert len(rows) == 6


def test_first_four_named_cases_are_the_issue_s():
    assert [n for n in ("removed_by_a_rejected_candidate", "cross_image_suppression", "cross_class_suppression", "cap_counted_across_images")
            if NAMED[n]["differs_from_textbook"]] == ["removed_by_a_rejected_candidate", "cross_image_suppression", "cross_class_suppression", "cap_counted_across_images"]


def test_second_block_scenario():
    """What tests/test_gpu_nms.py::test_members_in_a_wave_s_second_block_of_words relies on: in NC.second_block members past the first NMS_RESOLVE_THREADS * 64
    candidates are removed by and block later candidates, in a word that holds many members and in words that hold two, and a candidate's first blocker has
    removable members below it in the same word."""
    first = NC.NMS_RESOLVE_THREADS * 64
    boxes, scores = NC.second_block()
    trace = []
    selected = R.selection(R.candidates(boxes, scores, 0, 0.0), NC.SECOND_BLOCK_IOU, trace)
    late = [e for e in trace if e[2] >= first]
    assert all(p >= first for p, _, _ in late)
    word = lambda q: q // 64
    for w, packed in ((first // 64 + 1, True), (first // 64, False)):  # the dense word, a sparse word
        removed = [(p, q) for p, what, q in late if what == "removes" and word(q) == w]
        blocked = [(p, q) for p, what, q in late if what == "blocked by" and word(q) == w]
        assert removed and blocked, (w, removed, blocked)
        assert any(p == pb and q < qb for p, q in removed for pb, qb in blocked), w   # removed below the first blocker, by the same candidate, in the same word
    for w in (first // 64 + 16, first // 64 + 32):  # the other words of the same wave (16 waves: every 16th word)
        assert [e for e in late if word(e[2]) == w], w
    assert {what for _, what, q in late if word(q) == first // 64 + 32} == {"removes", "blocked by"}
    members = sorted(s[5] for s in selected)
    assert members[0] == 0 and len(members) == 23 and all(q >= first for q in members[1:])
    assert sum(word(q) == first // 64 + 1 for q in members) > 8   # the dense word stays dense


# ---------------------------------------------------------------------------------------------- 2. the Python host operator
def _recording():
    from rten_amd.recording import RecordingCtx

    class Ctx(RecordingCtx):
        def __init__(self):
            super().__init__()
            self.calls = []

        def call(self, name, *args):
            self.calls.append((name, args))
            super().call(name, *args)

    return Ctx()


def _refusal(op, inputs):
    from rten_amd import ops
    ctx = _recording()
    with pytest.raises(ops.OpError) as e:
        op.run(ctx, inputs(ctx) if callable(inputs) else inputs)
    assert ctx.calls == []  # refused before anything is launched
    return [e.value.kind, e.value.msg]


def test_python_operator_on_a_recording_context():
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    ctx = _recording()
    t = lambda *shape, dtype=F: DeviceTensor(ctx, shape, dtype)
    boxes, scores = t(2, 7, 4), t(2, 3, 7)
    val = lambda a: a.value if hasattr(a, "value") else a
    for center in (0, 1):
        for extra, tail in (([], [0, 0, 0.0, 0.0]), ([np.array([5], np.int64)], [1, 5, 0.0, 0.0]), ([np.array(2 ** 63 - 1, np.int64)], [1, 2 ** 31 - 1, 0.0, 0.0]),
                            ([np.array(-2 ** 63, np.int64)], [1, -2 ** 31, 0.0, 0.0]), ([None, np.array([[0.5]], F)], [0, 0, 0.5, 0.0]),
                            ([np.array(-1, I), None, np.array(0.25, F)], [1, -1, 0.0, 0.25]), ([None, None, None], [0, 0, 0.0, 0.0])):
            del ctx.calls[:]
            y = ops.NonMaxSuppression(center).run(ctx, [boxes, scores] + extra)[0]
            (name, args), = ctx.calls
            assert name == SYMBOL and y.dtype == np.dtype(I) and y.shape == (0, 3)  # (the recording context leaves the count at 0)
            assert [val(a) for a in args[:4]] == [center, 2, 3, 7] and [a.value for a in args[4:6]] == [boxes.ptr, scores.ptr]
            assert [val(a) for a in args[6:10]] == tail
    assert "NonMaxSuppression" in ops.OpRegistry.with_all_ops().op_types() and ops.NonMaxSuppression().max_inputs() == 5 and ops.NonMaxSuppression().batch_coupled()
    # empty: no launch
    del ctx.calls[:]
    assert ops.NonMaxSuppression().run(ctx, [t(2, 7, 4), t(2, 0, 7)])[0].shape == (0, 3) and ops.NonMaxSuppression().run(ctx, [t(2, 0, 4), t(2, 3, 0)])[0].shape == (0, 3)
    assert ctx.calls == []
    # every error, before any launch
    op = ops.NonMaxSuppression()
    assert _refusal(op, lambda c: [DeviceTensor(c, (1, 10, 3), F), DeviceTensor(c, (1, 10, 10), F)]) == GOLDEN["invalid"][1]["error"]
    assert _refusal(op, lambda c: [DeviceTensor(c, (1, 10, 4), F), DeviceTensor(c, (1, 10, 11), F)]) == GOLDEN["invalid"][0]["error"]
    assert _refusal(op, lambda c: [DeviceTensor(c, (2, 10, 4), F), DeviceTensor(c, (1, 10, 10), F)]) == GOLDEN["invalid"][0]["error"]
    assert _refusal(op, lambda c: [DeviceTensor(c, (1, 10, 4), F)]) == ["MissingInputs", ""]
    assert _refusal(op, lambda c: [DeviceTensor(c, (10, 4), F), DeviceTensor(c, (1, 10, 10), F)]) == ["InputCastFailed", "expected tensor with 3 dims"]
    assert _refusal(op, lambda c: [DeviceTensor(c, (1, 10, 4), I), DeviceTensor(c, (1, 10, 10), F)]) == ["InputCastFailed", "expected float32 tensor"]
    ok = lambda c: [DeviceTensor(c, (1, 10, 4), F), DeviceTensor(c, (1, 10, 10), F)]
    assert _refusal(op, lambda c: ok(c) + [np.array([1, 2], np.int64)]) == ["InputCastFailed", "expected tensor with 0 dims"]
    assert _refusal(op, lambda c: ok(c) + [np.array(0.5, F)]) == ["InputCastFailed", "expected int32 tensor"]
    assert _refusal(op, lambda c: ok(c) + [None, np.array(1, I)]) == ["InputCastFailed", "expected float32 tensor"]
    assert _refusal(op, lambda c: ok(c) + [None, None, np.zeros(0, F)]) == ["InputCastFailed", "expected tensor with 0 dims"]
    assert _refusal(op, lambda c: ok(c) + [None, None, None, None])[0] == "InvalidValue"
    assert _refusal(ops.NonMaxSuppression(2), ok) == ["InvalidValue", "center_point_box must be 0 or 1"]
    for i, what in ((2, "max_output_boxes_per_class"), (3, "iou_threshold"), (4, "score_threshold")):
        kind, msg = _refusal(op, lambda c: ok(c) + [None] * (i - 2) + [DeviceTensor(c, (1,), I if i == 2 else F)])
        assert kind == "UnsupportedValue" and what in msg and "device data" in msg, msg


# ---------------------------------------------------------------------------------------------- 3. header, ctypes, bindings
def test_header_ctypes_and_bindings_carry_the_symbols():
    from rten_amd import lib as L
    header = open(os.path.join(ROOT, "include", "rten_hip.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "rten-hip-sys", "src", "lib.rs")).read()
    assert "#define RTEN_HIP_ABI_VERSION 8\n" in header  # additive: the version stays
    assert re.search(r"int32_t " + SYMBOL + r"\(rten_hip_ctx \*ctx", header)
    assert SYMBOL in L.PROTOTYPES and L.PROTOTYPES[SYMBOL][0] is C.c_int32 and len(L.PROTOTYPES[SYMBOL][1]) == 13
    assert L.PROTOTYPES[SYMBOL][1][9] is C.c_float and L.PROTOTYPES[SYMBOL][1][10] is C.c_float
    line = bindings[bindings.index(f"pub fn {SYMBOL}(ctx: *mut rten_hip_ctx"):].split("\n")[0]
    assert "iou_threshold: f32" in line and "score_threshold: f32" in line and "count: *mut i64" in line and "selected: *mut i32" in line, line
    assert "rten_hip_model_run_eager" in L.PROTOTYPES and "pub fn rten_hip_model_run_eager(model: *mut rten_hip_model) -> i32;" in bindings
    comment = header[header.index("/* NonMaxSuppression"):header.index("int32_t " + SYMBOL)]
    for words in ("SYNCHRONISES", "CANNOT BE CAPTURED", "before it launches or copies anything", "Scratch", "`boxes` last dimension should have size 4",
                  "`boxes` and `scores` have incompatible shapes"):
        assert words in comment, words
    ops_header = open(os.path.join(ROOT, "include", "rten_hip_ops.hpp")).read()
    assert 'r.register_op<NonMaxSuppression>("NonMaxSuppression");' in ops_header
    kernels = open(os.path.join(ROOT, "rten_amd", "csrc", "nms.hip")).read()  # the geometry the GPU tests mirror
    for name, v in (("NMS_THREADS", NC.NMS_THREADS), ("NMS_SCAN_THREADS", NC.NMS_SCAN_THREADS), ("NMS_RESOLVE_THREADS", NC.NMS_RESOLVE_THREADS),
                    ("NMS_ORDER_THREADS", NC.NMS_ORDER_THREADS)):
        assert re.search(r"constexpr int " + name + r" = " + str(v) + r";", kernels), name


# ---------------------------------------------------------------------------------------------- 4. the loader's checks, through the CLI
def _parse_only(tmp_path, name, data):
    from tests.test_graph_executor import run_cli
    p = tmp_path / name
    p.write_bytes(data)
    return run_cli("--parse-only", str(p))


def _nms_lines(out):
    return [ln.strip() for ln in out.stdout.splitlines() if ln.strip().startswith("nms step")]


def test_cli_prints_the_step_line_of_the_detector_head(tmp_path):
    """Fails on a tree without the operator: its --parse-only prints no `nms step` line (and its loader refuses the graph: "operator NonMaxSuppression is
    not available on the HIP backend")."""
    from rten_amd import onnx_writer as ow
    tail = "; reads the row count back (eager runs only, no capture, no sub-batch chains)"
    for kw, line in ((dict(), 'nms step "nms": [y1, x1, y2, x2] boxes, max_output_boxes_per_class absent (no limit), iou_threshold from input 3, score_threshold 0'),
                     (dict(center_point_box=1, max_output_boxes_per_class=2 ** 63 - 1, score_threshold=0.3),
                      'nms step "nms": [cx, cy, w, h] boxes, max_output_boxes_per_class from input 2, iou_threshold from input 3, score_threshold from input 4'),
                     (dict(iou_threshold=None, score_threshold=0.2, batch=4),
                      'nms step "nms": [y1, x1, y2, x2] boxes, max_output_boxes_per_class absent (no limit), iou_threshold 0, score_threshold from input 4'),
                     (dict(iou_threshold=None), 'nms step "nms": [y1, x1, y2, x2] boxes, max_output_boxes_per_class absent (no limit), iou_threshold 0, score_threshold 0')):
        out = _parse_only(tmp_path, "head.onnx", ow.detector_head_graph(**kw)[0])
        assert out.returncode == 0, out.stderr
        assert "NonMaxSuppression x1" in out.stdout and _nms_lines(out) == [line + tail], out.stdout


@pytest.mark.parametrize("bad,words", [("center_point_box_2", ("NonMaxSuppression nms", "center_point_box 2 is not 0")),
                                       ("six_inputs", ("NonMaxSuppression nms", "takes at most 5 inputs (it has 6)")),
                                       ("max_input", ("NonMaxSuppression nms", "max_output_boxes_per_class must be a constant or computable from the input shapes", '"max_per_class_in"')),
                                       ("iou_input", ("NonMaxSuppression nms", "iou_threshold must be a constant or computable from the input shapes", '"iou_thr_in"')),
                                       ("score_input", ("NonMaxSuppression nms", "score_threshold must be a constant or computable from the input shapes", '"score_thr_in"'))])
def test_cli_refuses_by_node_name(tmp_path, bad, words):
    from rten_amd import onnx_writer as ow
    out = _parse_only(tmp_path, "bad.onnx", ow.detector_head_graph(bad=bad)[0])
    assert out.returncode == 1 and all(w in out.stderr for w in words), out.stdout + out.stderr
