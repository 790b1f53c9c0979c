"""NonMaxSuppression on the device: rten_hip_non_max_suppression_f32 (rten_amd/csrc/nms.hip) row for row against the reference's rule (tests/nms_rules.py)
-- candidate counts around every word of the alive vector, past a word per wave and past a word per thread, guarded and misaligned operands, rows past the count
untouched, the named cases that tell the rule from textbook NMS --, the Python operator, and onnx_writer.detector_head_graph through one loaded Graph at
two batch sizes in both orders, the CLI node by node / fused / unfused, the C-ABI model and its clone, and every refusal: sub-batch chains, and a capture
decided from the plan before any capture begins."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import confine as K
from tests import nms_cases as NC
from tests import nms_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
pytestmark = pytest.mark.gpu


def nms(ctx, boxes, scores, center_point_box=0, max_output_boxes_per_class=None, iou_threshold=0.0, score_threshold=0.0, leads=(1, 2, 3), what=""):
    """The raw entry point on guarded boxes / scores / rows, each `lead` elements off a 16-byte boundary -> the rows, after checking that they are the rule's
    and that nothing but the first `count` rows was written."""
    n, b, _ = boxes.shape
    c = scores.shape[1]
    bg, sg, out = K.Guarded(ctx, boxes, lead=leads[0]), K.Guarded(ctx, scores, lead=leads[1]), K.Guarded(ctx, max(n * b, 1) * 12, lead=leads[2])
    count = C.c_int64(-1)
    cap = max_output_boxes_per_class
    ctx.call("rten_hip_non_max_suppression_f32", center_point_box, n, c, b, bg.vp, sg.vp, 0 if cap is None else 1, 0 if cap is None else int(cap),
             C.c_float(iou_threshold), C.c_float(score_threshold), out.vp, C.byref(count))
    what = f"nms {what} N {n} B {b} C {c} center {center_point_box} cap {cap} iou {iou_threshold} score {score_threshold} leads {leads}"
    want = rule_rows(boxes, scores, center_point_box, cap, iou_threshold, score_threshold)
    assert count.value == len(want), f"{what}: {count.value} rows instead of {len(want)}"
    got = out.check(out.raw(), (count.value, 3), K.dense((count.value, 3)), I, what)  # the rows past `count` still hold the fill
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} rows differ, first row {bad[0]}: {got[bad[0]].tolist()} instead of {want[bad[0]].tolist()}"
    for g in (bg, sg):
        g.check(g.raw(), g_shape(g), K.dense(g_shape(g)), F, what + " (an operand)")
    return got


_SELECTIONS = {}


def rule_rows(boxes, scores, center_point_box, cap, iou_threshold, score_threshold):
    """R.non_max_suppression, with the sorted selection -- the Python loop -- computed once per input and thresholds and shared by the caps applied to it."""
    R.check_shapes(boxes.shape, scores.shape)
    key = (boxes.tobytes(), scores.tobytes(), boxes.shape, scores.shape, center_point_box, float(iou_threshold), float(score_threshold))
    if key not in _SELECTIONS:
        _SELECTIONS.clear()  # (one entry: consecutive calls share it)
        _SELECTIONS[key] = R.sorted_selection(boxes, scores, center_point_box, iou_threshold, score_threshold)
    return R.capped_rows(_SELECTIONS[key], cap)


def g_shape(g):
    return (g.nbytes // 4,)


def with_candidates(scores, k, seed):
    """The same scores with exactly `k` boxes (over all images) whose best class reaches 0.5."""
    n, c, b = scores.shape
    rng = np.random.default_rng(seed)
    passing = np.zeros(n * b, bool)
    passing[rng.choice(n * b, k, replace=False)] = True
    s = np.where(passing.reshape(n, 1, b), F(0.5) + scores * F(0.5), scores * F(0.4)).astype(F)
    assert len(R.candidates(np.zeros((n, b, 4), F), s, 0, 0.5)) == k
    return s


# ================================================================================================ the entry point
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 129])
@pytest.mark.parametrize("center", [0, 1])
def test_candidate_counts_around_a_word_of_alive(ctx, k, center):
    boxes, scores = NC.grid_boxes(100 + k, 1, NC.NMS_THREADS + 1, 2, center=bool(center), spread=16)
    nms(ctx, boxes, with_candidates(scores, k, k), center, None, 0.5, 0.5, what=f"{k} candidates")


@pytest.mark.parametrize("n,b,c", [(1, 1, 1), (3, 1, 2), (1, NC.NMS_THREADS + 1, 1), (3, NC.NMS_THREADS + 1, 81), (2, 3 * NC.NMS_THREADS - 1, 2)])
@pytest.mark.parametrize("center", [0, 1])
def test_shapes_thresholds_and_caps(ctx, n, b, c, center):
    repeat = 40 if b > 100 else 0  # (copies of the first boxes: pairs whose iou is exactly 1)
    boxes, scores = NC.grid_boxes(7 * n + b + c, n, b, c, center=bool(center), repeat=repeat)
    heavy = n * b > NC.NMS_THREADS + 1  # (the rule is a Python loop, quadratic where little is suppressed: the full grid up to one image of B one past a workgroup)
    for iou in ((0.5,) if heavy else (0.0, 0.5, 1.0)):
        for score in ((0.6,) if heavy else (-1.0, 0.6, 2.0)):  # drops none, some, all
            for cap in (None, 1):
                got = nms(ctx, boxes, scores, center, cap, iou, score)
                if repeat and not heavy and iou == 1.0 and score < 0 and cap is None:
                    assert 0 < len(got) < n * b  # `iou >= 1` did hit: a copy was rejected, or replaced what it copies
    for cap in (0, -1, 2, 2 ** 31 - 1):
        nms(ctx, boxes, scores, center, cap, 0.5, 0.6 if heavy else 0.3)  # (shares the selection of the loop above where the shape is large)


@pytest.mark.parametrize("leads", [(0, 0, 0), (1, 1, 1), (3, 2, 1), (2, 3, 3)])
def test_misaligned_operands(ctx, leads):
    boxes, scores = NC.grid_boxes(5, 2, 70, 3)
    nms(ctx, boxes, scores, 0, 3, 0.5, 0.2, leads=leads)


# (the [cx, cy, w, h] form of a NaN corner is another box: those cases run in corner order only)
NAMED = [(name, center) for name, case in sorted(NC.named_cases().items()) for center in (0, 1) if center == 0 or np.isfinite(case["boxes"]).all()]


@pytest.mark.parametrize("name,center", NAMED)
def test_named_cases(ctx, name, center):
    case = NC.named_cases()[name]
    boxes = NC.to_center(case["boxes"]) if center else case["boxes"]
    got = nms(ctx, boxes, case["scores"], center, case["kw"].get("max_output_boxes_per_class"), case["kw"].get("iou_threshold", 0.0),
              case["kw"].get("score_threshold", 0.0), what=name)
    if not center:
        assert np.array_equal(got, R.non_max_suppression(case["boxes"], case["scores"], **case["kw"]))


def test_several_words_of_alive_per_wave(ctx):
    b = NC.NMS_RESOLVE_THREADS // 64 * 64 * 16 + 70  # 17 words per wave
    boxes, scores = NC.clustered(b, b)
    got = nms(ctx, boxes, scores, 0, None, 0.5, 0.0, what="17 words of alive per wave")
    assert 1 <= len(got) <= 3


def test_members_in_a_wave_s_second_block_of_words(ctx):
    """Past NMS_RESOLVE_THREADS * 64 candidates a wave owns more than 64 words of `alive`, and what a candidate removes from the later ones travels through
    memory.  NC.second_block puts members there, packed in one word (the dense form) and spread over three words of one wave (the sparse form), and then
    candidates that remove them, that are blocked by them, and whose first blocker has removable members below it in the same word
    (tests/test_nms_ops.py::test_second_block_scenario shows on the CPU that each of these happens)."""
    boxes, scores = NC.second_block()
    for center in (0, 1):
        got = nms(ctx, NC.to_center(boxes) if center else boxes, scores, center, None, NC.SECOND_BLOCK_IOU, 0.0, what="second block of words")
        assert len(got) == 23 and (got[:, 2] >= NC.NMS_RESOLVE_THREADS * 64).sum() == 22


def test_empty_inputs_and_bad_arguments(ctx):
    from rten_amd import lib as L
    count = C.c_int64(-1)
    buf = K.Guarded(ctx, 64)
    for n, c, b in ((0, 3, 5), (2, 0, 5), (2, 3, 0)):
        ctx.call("rten_hip_non_max_suppression_f32", 0, n, c, b, buf.vp, buf.vp, 0, 0, C.c_float(0.5), C.c_float(0), buf.vp, C.byref(count))
        assert count.value == 0
        count.value = -1
    buf.check(buf.raw(), (0,), (1,), I, "empty inputs launch nothing")
    for args in ((2, 1, 1, 1), (0, -1, 1, 1), (0, 1, 1, 2 ** 31)):
        with pytest.raises(L.HipError):
            ctx.call("rten_hip_non_max_suppression_f32", *args, buf.vp, buf.vp, 0, 0, C.c_float(0.5), C.c_float(0), buf.vp, C.byref(count))
    with pytest.raises(L.HipError):
        ctx.call("rten_hip_non_max_suppression_f32", 0, 1, 1, 1, buf.vp, buf.vp, 0, 0, C.c_float(0.5), C.c_float(0), buf.vp, None)


def test_refused_inside_a_capture_before_anything_is_launched(ctx):
    from rten_amd import lib as L
    boxes, scores = NC.grid_boxes(9, 1, 40, 2)
    bg, sg, out = K.Guarded(ctx, boxes), K.Guarded(ctx, scores), K.Guarded(ctx, 40 * 12)
    count = C.c_int64(-7)
    ctx.sync()
    ctx.graph_begin()
    try:
        with pytest.raises(L.HipError) as e:
            ctx.call("rten_hip_non_max_suppression_f32", 0, 1, 2, 40, bg.vp, sg.vp, 0, 0, C.c_float(0.5), C.c_float(0), out.vp, C.byref(count))
    finally:
        ctx.call("rten_hip_graph_abort")  # the capture ends here; nothing was recorded into it
    assert "cannot be captured" in str(e.value) and count.value == -7
    ctx.sync()
    out.check(out.raw(), (0,), (1,), I, "a refused call writes nothing")
    nms(ctx, boxes, scores, 0, None, 0.5, 0.0, what="after the refusal")


def test_python_operator_on_the_device(ctx):
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    dev = lambda a: DeviceTensor.from_numpy(ctx, np.ascontiguousarray(a))
    boxes, scores = NC.grid_boxes(21, 2, 90, 4)
    for center in (0, 1):
        bx = NC.to_center(boxes) if center else boxes
        for extra, kw in (([], {}), ([np.array([2], np.int64)], {"max_output_boxes_per_class": 2}),
                          ([None, np.array([0.5], F)], {"iou_threshold": 0.5}),
                          ([np.array(2 ** 63 - 1, np.int64), np.array(0.5, F), np.array(0.4, F)], {"max_output_boxes_per_class": 2 ** 31 - 1, "iou_threshold": 0.5, "score_threshold": 0.4})):
            y = ops.NonMaxSuppression(center).run(ctx, [dev(bx), dev(scores)] + extra)[0]
            want = R.non_max_suppression(bx, scores, center, **kw)
            assert y.dtype == np.dtype(I) and y.shape == want.shape and np.array_equal(y.numpy(), want), (center, kw)
    assert ops.NonMaxSuppression().run(ctx, [dev(np.zeros((2, 5, 4), F)), dev(np.zeros((2, 0, 5), F))])[0].shape == (0, 3)


# ================================================================================================ the detector head graph
from tests.test_gpu_sample import SESSION_TIMEOUT_S  # noqa: E402


def head_feeds(seed, batch, features=6, h=5, w=7):
    return {"x": np.random.default_rng(seed).normal(0, 1, (batch, features, h, w)).astype(F)}


def session_runs(tmp_path, data, feeds_list):
    """ONE loaded Graph in one process of tests/cpp/graph_session.cpp: an eager run at every binding, in order -> [{output: array}]."""
    from safetensors.numpy import save_file
    from tests import graph_sessions as gs
    from tests.test_gpu_graph_fuzz import read_safetensors
    d = str(tmp_path)
    open(os.path.join(d, "session.onnx"), "wb").write(data)
    lines = []
    for k, feeds in enumerate(feeds_list):
        save_file({nm: np.ascontiguousarray(a) for nm, a in feeds.items()}, os.path.join(d, f"b{k}.safetensors"))
        lines.append(f"run {os.path.join(d, f'b{k}.safetensors')} {os.path.join(d, f'out{k}.safetensors')}")
    open(os.path.join(d, "script.txt"), "w").write("\n".join(lines) + "\n")
    r = subprocess.run([gs.build_session_probe(), os.path.join(d, "session.onnx"), os.path.join(d, "script.txt")], capture_output=True, text=True, timeout=SESSION_TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return [dict(read_safetensors(os.path.join(d, f"out{k}.safetensors"))) for k in range(len(feeds_list))]


def check_head_outputs(got, kw, what, batch, locations=35, classes=3):
    """selected is the rule's answer for the boxes and scores the SAME run produced, picked the rows of image 0's boxes it names."""
    boxes, scores = got["boxes"].view(F).reshape(batch, locations, 4), got["scores"].view(F).reshape(batch, classes, locations)
    want = R.non_max_suppression(boxes, scores, kw.get("center_point_box", 0), kw.get("max_output_boxes_per_class"), kw.get("iou_threshold") or 0.0,
                                 kw.get("score_threshold") or 0.0)
    if kw.get("max_output_boxes_per_class") is not None:
        want = R.non_max_suppression(boxes, scores, kw.get("center_point_box", 0), R.saturate_i32(kw["max_output_boxes_per_class"]), kw.get("iou_threshold") or 0.0,
                                     kw.get("score_threshold") or 0.0)
    sel = got["selected"].view(I).reshape(-1, 3)
    assert sel.shape == want.shape and np.array_equal(sel, want), (what, sel.tolist()[:5], want.tolist()[:5])
    if (kw.get("score_threshold") or 0.0) > 1.0:
        assert len(want) == 0 and picked_shape_ok(got), what  # (every score is a sigmoid: nothing passes, and the Gathers behind the node see [0, 3])
        return sel
    assert len(want) > (1 if kw.get("iou_threshold") else 0), what  # (an absent iou_threshold is 0: every finite pair overlaps, one row survives)
    picked = got["picked"].view(F).reshape(-1, 4)
    assert np.array_equal(picked.view(np.uint32), boxes[0][want[:, 2]].view(np.uint32)), what
    return sel


def picked_shape_ok(got):
    return got["picked"].size == 0


HEAD_FORMS = [dict(center_point_box=0, iou_threshold=0.5), dict(center_point_box=1, max_output_boxes_per_class=2 ** 63 - 1, iou_threshold=0.45, score_threshold=0.3),
              dict(center_point_box=1, max_output_boxes_per_class=2, iou_threshold=None, score_threshold=0.2),
              dict(center_point_box=0, iou_threshold=0.5, score_threshold=2.0)]  # (drops every box: count == 0)
HEAD_OUTPUTS = ["selected", "picked", "boxes", "scores"]


@pytest.mark.parametrize("form", range(len(HEAD_FORMS)))
def test_detector_head_through_one_loaded_graph(ctx, tmp_path, form):
    from rten_amd import onnx_writer as ow
    kw = HEAD_FORMS[form]
    data, _ = ow.detector_head_graph(expose_operands=True, **kw)
    feeds = [head_feeds(1, 2), head_feeds(2, 5), head_feeds(3, 2), head_feeds(4, 5)]  # two batch sizes, in both orders
    counts = [len(check_head_outputs(got, kw, f"one graph, binding {k}", (2, 5, 2, 5)[k])) for k, got in enumerate(session_runs(tmp_path, data, feeds))]
    assert len(set(counts)) > 1 or not kw.get("iou_threshold") or kw.get("score_threshold") == 2.0, counts  # the output shape did change from run to run


@pytest.mark.parametrize("extra", [("-t",), (), ("--no-fuse",)], ids=["node by node", "fused", "unfused"])
def test_detector_head_through_the_cli(ctx, tmp_path, extra):
    from rten_amd import onnx_writer as ow
    from tests.test_gpu_sample import run_cli_graph
    kw = HEAD_FORMS[1]
    data, _ = ow.detector_head_graph(expose_operands=True, **kw)
    got, log = run_cli_graph(tmp_path, data, head_feeds(5, 3), HEAD_OUTPUTS, {"batch": 3, "h": 5, "w": 7}, extra)
    check_head_outputs(got, kw, f"cli {extra}", 3)
    assert 'nms step "nms": [cx, cy, w, h] boxes' in log
    if extra == ("-t",):
        assert "NonMaxSuppression" in log


def test_cli_refuses_to_capture_by_node_name(ctx, tmp_path):
    from rten_amd import onnx_writer as ow
    from tests.test_graph_executor import run_cli
    data, _ = ow.detector_head_graph()
    path = tmp_path / "model.onnx"
    path.write_bytes(data)
    r = run_cli("--graph", "-s", "batch=2", "-s", "h=5", "-s", "w=7", str(path))
    assert r.returncode != 0 and 'NonMaxSuppression "nms"' in r.stderr and "cannot be captured" in r.stderr, r.stdout[-1500:] + r.stderr[-1500:]
    assert "Captured" not in r.stdout


def model_rows(ctx, m, feeds):
    from rten_amd.tensor import DeviceTensor
    for name in m.inputs:
        a = feeds[name]
        DeviceTensor(ctx, a.shape, a.dtype, ptr=m.bind_input(name, a.shape), keepalive=m).upload(a)
    ctx.sync()
    m.run_eager()
    m.sync()
    out = {}
    for i, name in enumerate(m.outputs):
        ptr, shape = m.output(i)
        out[name] = DeviceTensor(ctx, shape, m.output_dtype(i), ptr=ptr, keepalive=m).numpy()
    return out


def test_c_abi_model_refuses_capture_then_runs_eagerly_and_so_does_its_clone(ctx):
    from rten_amd import lib as L
    from rten_amd import onnx_writer as ow
    kw = HEAD_FORMS[1]
    data, _ = ow.detector_head_graph(expose_operands=True, **kw)
    m, other = L.Model(ctx, data), L.Context(0)
    try:
        first = check_head_outputs(model_rows(ctx, m, head_feeds(6, 2)), kw, "the C-ABI model, eager", 2)
        assert ctx.lib.rten_hip_capture_active(ctx.h) == 0
        with pytest.raises(L.HipError) as e:
            m.prepare()  # prepare captures: refused from the plan, before any capture begins
        assert 'NonMaxSuppression "nms"' in str(e.value) and "cannot be captured" in str(e.value), str(e.value)
        assert ctx.lib.rten_hip_capture_active(ctx.h) == 0
        again = check_head_outputs(model_rows(ctx, m, head_feeds(6, 2)), kw, "the same model after the refusal", 2)
        assert np.array_equal(first, again)
        with pytest.raises(L.HipError) as e:
            m.bind_input("x", (5, 6, 5, 7))  # another batch size without unbind: the rule for every model
        assert "same dim 0" in str(e.value)
        m.unbind()
        with pytest.raises(L.HipError):
            m.run_eager()  # nothing is bound
        check_head_outputs(model_rows(ctx, m, head_feeds(7, 5)), kw, "the same model at another batch size", 5)
        lane = m.clone(other)
        try:
            rows = check_head_outputs(model_rows(other, lane, head_feeds(6, 2)), kw, "its clone on a second context", 2)
            assert np.array_equal(first, rows)
        finally:
            lane.close()
    finally:
        m.close()
        other.close()


def test_sub_batch_chains_are_refused(ctx):
    from rten_amd import lib as L
    from rten_amd import onnx_writer as ow
    data, _ = ow.detector_head_graph()
    with pytest.raises(L.HipError) as e:
        L.Model(ctx, data, None, 2)
    assert 'NonMaxSuppression "nms"' in str(e.value) and "couples the rows" in str(e.value), str(e.value)
