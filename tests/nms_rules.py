"""The reference's NonMaxSuppression (src/ops/non_max_suppression.rs:40-188) restated as written: a plain Python loop over numpy float32 scalars.  It is
the rule the kernels of rten_amd/csrc/nms.hip and the host layers are held to, row for row -- and it is NOT textbook score-sorted per-class NMS:

  * candidates are taken in (n, b) order, not by score; a box's class is the arg-max over scores[n, :, b] under f32::total_cmp with the LAST maximal
    class (Iterator::max_by), and it is dropped when max_score < score_threshold (an IEEE compare: a NaN score stays);
  * the "union" of the IoU is the bounding hull; min / max ignore a NaN operand (np.fmin / np.fmax, never np.minimum); 0 / 0 = NaN compares false;
  * ONE selected list serves every image and every class.  A candidate walks it in order: at a member with iou >= iou_threshold it removes the member
    when its own score is greater and goes on, otherwise it is rejected and the walk stops -- members removed earlier in the walk stay removed;
  * the list is stably sorted by score descending under total_cmp; with a cap the first `max` rows of each class are kept, counted over the whole
    batch (a negative or zero cap keeps nothing); an absent cap is no limit.

Errors are (kind, message) of the reference's OpError."""
import numpy as np

F = np.float32
INT32_MAX = 2 ** 31 - 1


class RuleError(Exception):
    def __init__(self, kind, msg):
        super().__init__(f"{kind}({msg!r})")
        self.kind, self.msg = kind, msg


def total_key(x):
    """f32::total_cmp as an integer key (ascending): -NaN < -Inf < ... < -0 < +0 < ... < +Inf < +NaN."""
    u = int(np.asarray(x, F).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def saturate_i32(v):
    """The loader's int64 -> int32 narrowing (onnx_loader.rs: saturating_cast_i64_to_i32): an exporter's INT64_MAX becomes INT32_MAX."""
    return max(-2 ** 31, min(INT32_MAX, int(v)))


def area(t, l, b, r):
    return F(np.fmax(F(b - t), F(0)) * np.fmax(F(r - l), F(0)))


def iou(a, o):
    """a, o: [t, l, b, r] float32 scalars."""
    hull = (np.fmin(a[0], o[0]), np.fmin(a[1], o[1]), np.fmax(a[2], o[2]), np.fmax(a[3], o[3]))
    inter = (np.fmax(a[0], o[0]), np.fmax(a[1], o[1]), np.fmin(a[2], o[2]), np.fmin(a[3], o[3]))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return F(area(*inter) / area(*hull))


def corners(c, center_point_box):
    c0, c1, c2, c3 = (F(v) for v in c)
    if not center_point_box:
        return (c0, c1, c2, c3)
    x, y, w, h = c0, c1, c2, c3
    with np.errstate(invalid="ignore", over="ignore"):
        return (F(y - F(h / F(2))), F(x - F(w / F(2))), F(y + F(h / F(2))), F(x + F(w / F(2))))


def candidates(boxes, scores, center_point_box=0, score_threshold=0.0):
    """[(tlbr, n, b, class, score)] in (n, b) order."""
    thr = F(score_threshold)
    out = []
    N, C, B = scores.shape
    for n in range(N):
        keys = np.where(scores[n].view(np.uint32) & 0x80000000, ~scores[n].view(np.uint32), scores[n].view(np.uint32) | np.uint32(0x80000000))  # [C, B]
        last_max = C - 1 - np.argmax(keys[::-1], axis=0)   # the last maximal class of each box
        for b in range(B):
            cls = int(last_max[b])
            assert keys[cls, b] == total_key(scores[n, cls, b])
            score = scores[n, cls, b]
            if score < thr:
                continue
            out.append((corners(boxes[n, b], center_point_box), n, b, cls, score))
    return out


def check_shapes(boxes_shape, scores_shape):
    if boxes_shape[2] != 4:
        raise RuleError("InvalidValue", "`boxes` last dimension should have size 4")
    if boxes_shape[0] != scores_shape[0] or boxes_shape[1] != scores_shape[2]:
        raise RuleError("IncompatibleInputShapes", "`boxes` and `scores` have incompatible shapes")


def selection(cands, iou_threshold, trace=None):
    """The selection loop on candidates(): the selected list before the sort.  `trace` (a list) receives (candidate position, "removes" | "blocked by",
    member position) for every removal and rejection, positions counting the candidates in order."""
    thr = F(iou_threshold)
    selected = []
    for pos, cand in enumerate(cands):
        cand = cand + (pos,)
        keep = True
        i = 0
        while i < len(selected):
            other = selected[i]
            if iou(cand[0], other[0]) >= thr:
                if cand[4] > other[4]:
                    if trace is not None:
                        trace.append((pos, "removes", other[5]))
                    del selected[i]
                else:
                    if trace is not None:
                        trace.append((pos, "blocked by", other[5]))
                    keep = False
                    break
            else:
                i += 1
        if keep:
            selected.append(cand)
    return selected


def non_max_suppression(boxes, scores, center_point_box=0, max_output_boxes_per_class=None, iou_threshold=0.0, score_threshold=0.0):
    """-> int32 [count, 3] rows [n, class, b]."""
    boxes, scores = np.ascontiguousarray(boxes, F), np.ascontiguousarray(scores, F)
    assert boxes.ndim == 3 and scores.ndim == 3
    check_shapes(boxes.shape, scores.shape)
    if scores.shape[1] == 0:
        return np.zeros((0, 3), np.int32)
    return capped_rows(sorted_selection(boxes, scores, center_point_box, iou_threshold, score_threshold), max_output_boxes_per_class)


def sorted_selection(boxes, scores, center_point_box=0, iou_threshold=0.0, score_threshold=0.0):
    """The selected list after the stable sort by score descending (what the cap is then applied to)."""
    selected = selection(candidates(np.ascontiguousarray(boxes, F), np.ascontiguousarray(scores, F), center_point_box, score_threshold), iou_threshold)
    selected.sort(key=lambda s: -total_key(s[4]))   # list.sort is stable: ties keep (n, b) order
    return selected


def capped_rows(selected, max_output_boxes_per_class=None):
    if max_output_boxes_per_class is not None:
        cap, counts, kept = int(max_output_boxes_per_class), {}, []
        for s in selected:
            if counts.get(s[3], 0) >= cap:
                continue
            counts[s[3]] = counts.get(s[3], 0) + 1
            kept.append(s)
        selected = kept
    return np.array([[s[1], s[3], s[2]] for s in selected], np.int32).reshape(-1, 3)
