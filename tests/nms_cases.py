"""Inputs for the NonMaxSuppression tests (CPU: tests/test_nms_ops.py, device: tests/test_gpu_nms.py): the named cases that tell the reference's rule
(tests/nms_rules.py) from textbook NMS, a textbook restatement to tell them apart with, and seeded boxes on a grid of eighths."""
import numpy as np

from tests import nms_rules as R

F = np.float32
# rten_amd/csrc/nms.hip
NMS_THREADS, NMS_SCAN_THREADS, NMS_RESOLVE_THREADS, NMS_ORDER_THREADS = 256, 1024, 1024, 1024


def textbook(boxes, scores, max_output_boxes_per_class=None, iou_threshold=0.0, score_threshold=0.0):
    """Score-sorted, per-image, per-class NMS with the set-union IoU on [y1, x1, y2, x2] boxes (a box's class is its best class): what the reference does
    NOT compute.  -> rows [n, class, b] sorted by (n, class, score descending)."""
    boxes, scores = np.asarray(boxes, np.float64), np.asarray(scores, np.float64)
    rows = []

    def iou(a, o):
        inter = max(min(a[2], o[2]) - max(a[0], o[0]), 0) * max(min(a[3], o[3]) - max(a[1], o[1]), 0)
        union = (a[2] - a[0]) * (a[3] - a[1]) + (o[2] - o[0]) * (o[3] - o[1]) - inter
        return inter / union if union > 0 else 0.0

    for n in range(scores.shape[0]):
        cls = np.argmax(scores[n], axis=0)
        for c in range(scores.shape[1]):
            ids = [b for b in range(scores.shape[2]) if cls[b] == c and scores[n, c, b] >= score_threshold]
            ids.sort(key=lambda b: -scores[n, c, b])
            kept = []
            for b in ids:
                if all(iou(boxes[n, b], boxes[n, k]) < iou_threshold for k in kept):
                    kept.append(b)
            if max_output_boxes_per_class is not None:
                kept = kept[:max(int(max_output_boxes_per_class), 0)]
            rows += [[n, c, b] for b in kept]
    return np.array(rows, np.int32).reshape(-1, 3)


def _case(boxes, scores, differs_from_textbook=False, **kw):
    return {"boxes": np.asarray(boxes, F), "scores": np.asarray(scores, F), "kw": kw, "differs_from_textbook": differs_from_textbook}


def named_cases():
    """name -> {boxes [N, B, 4] (y1, x1, y2, x2), scores [N, C, B], kw (the rule's keyword arguments), differs_from_textbook}."""
    nan, inf = np.nan, np.inf
    c = {}
    # the selected list is [A .3, D .8]; X (.5) covers both: it removes A (.5 > .3), is then rejected by D -- and A stays removed.  Textbook keeps D and A.
    c["removed_by_a_rejected_candidate"] = _case([[[0, 0, 10, 10], [0, 20, 10, 30], [0, 0, 10, 30]]], [[[0.3, 0.8, 0.5]]], True, iou_threshold=0.3)
    # one selected list for all images: the same box in image 1 is rejected by image 0's (equal scores), or replaces it (a higher score)
    c["cross_image_suppression"] = _case([[[0, 0, 10, 10]], [[0, 0, 10, 10]]], [[[0.6]], [[0.6]]], True, iou_threshold=0.5)
    c["cross_image_replacement"] = _case([[[0, 0, 10, 10]], [[0, 0, 10, 10]]], [[[0.6]], [[0.7]]], True, iou_threshold=0.5)
    # ... and for all classes
    c["cross_class_suppression"] = _case([[[0, 0, 10, 10], [1, 1, 11, 11]]], [[[0.9, 0.1], [0.2, 0.8]]], True, iou_threshold=0.5)
    # the cap counts over the whole batch: one row of class 0 in all, not one per image
    c["cap_counted_across_images"] = _case([[[0, 0, 10, 10]], [[50, 50, 60, 60]]], [[[0.6]], [[0.7]]], True, iou_threshold=0.5, max_output_boxes_per_class=1)
    # the bounding hull, not the set union: 25 / 225 < 0.125 <= 25 / 175
    c["hull_versus_union"] = _case([[[0, 0, 10, 10], [5, 5, 15, 15]]], [[[0.9, 0.8]]], True, iou_threshold=0.125)
    # equal scores keep (n, b) order through the stable sort
    c["ties_in_score"] = _case([[[0, 0, 1, 1], [0, 5, 1, 6], [0, 10, 1, 11]], [[5, 0, 6, 1], [5, 5, 6, 6], [5, 10, 6, 11]]],
                               [[[0.5, 0.7, 0.5]], [[0.7, 0.5, 0.7]]], iou_threshold=0.5)
    # equal class scores: the LAST maximal class
    c["class_ties_last_wins"] = _case([[[0, 0, 1, 1], [0, 5, 1, 6], [0, 10, 1, 11]]], [[[0.5, 0.2, 0.9], [0.5, 0.7, 0.1], [0.5, 0.7, 0.9]]], iou_threshold=0.5)
    # total_cmp: -0 < +0
    c["signed_zero_class_scores"] = _case([[[0, 0, 1, 1], [0, 5, 1, 6], [0, 10, 1, 11], [0, 15, 1, 16]]],
                                          [[[0.0, -0.0, -0.0, 0.0], [-0.0, 0.0, -0.0, 0.0]]], iou_threshold=0.5)
    # +NaN is above +Inf, -NaN below -Inf; a NaN score is not dropped by the threshold; `cand > member` is false with a NaN on either side
    neg_nan = np.array([0xFFC00000], np.uint32).view(F)[0]
    c["nan_scores"] = _case([[[0, 0, 10, 10], [0, 0, 10, 10], [0, 20, 10, 30], [0, 20, 10, 30], [0, 40, 10, 50]]],
                            [[[nan, 0.9, 0.4, nan, neg_nan], [inf, 0.1, 0.3, 0.2, -inf]]], iou_threshold=0.5, score_threshold=0.25)
    # a NaN coordinate is ignored by min / max
    c["nan_coordinates"] = _case([[[0, 0, 10, 10], [nan, 0, 10, 10], [0, nan, nan, 10], [nan, nan, nan, nan], [0, 0, 10, 10]]], [[[0.5, 0.6, 0.4, 0.7, 0.3]]],
                                 iou_threshold=0.5)
    # 0 / 0 = NaN: never >= the threshold, even 0
    c["degenerate_boxes"] = _case([[[5, 5, 5, 5], [5, 5, 5, 5], [0, 0, 10, 10], [7, 7, 3, 3], [0, 0, 10, 10]]], [[[0.5, 0.6, 0.7, 0.8, 0.2]]], iou_threshold=0.0)
    c["degenerate_only"] = _case([[[5, 5, 5, 5], [5, 5, 5, 5], [5, 5, 5, 5]]], [[[0.5, 0.6, 0.4]]], iou_threshold=0.0)   # all three stay: NaN >= 0 is false
    disjoint = [[[0, 6 * k, 1, 6 * k + 1] for k in range(6)]]
    sc = [[[0.1, 0.9, 0.3, 0.8, 0.2, 0.7], [0.6, 0.2, 0.5, 0.1, 0.4, 0.3]]]
    c["negative_cap"] = _case(disjoint, sc, iou_threshold=0.5, max_output_boxes_per_class=-1)
    c["zero_cap"] = _case(disjoint, sc, iou_threshold=0.5, max_output_boxes_per_class=0)
    c["cap_of_two"] = _case(disjoint, sc, iou_threshold=0.5, max_output_boxes_per_class=2)
    c["absent_cap"] = _case(disjoint, sc, iou_threshold=0.5)
    c["saturated_cap"] = _case(disjoint, sc, iou_threshold=0.5, max_output_boxes_per_class=R.saturate_i32(2 ** 63 - 1))
    return c


def to_center(boxes):
    """[y1, x1, y2, x2] -> [cx, cy, w, h] as the reference's own test helper does (non_max_suppression.rs:264-273)."""
    b = np.asarray(boxes, F)
    t, l, bt, r = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([((l + r) / F(2)).astype(F), ((t + bt) / F(2)).astype(F), (r - l).astype(F), (bt - t).astype(F)], axis=-1).astype(F)


def grid_boxes(seed, n, b, c, center=False, spread=8, repeat=0):
    """Boxes whose corners sit on a grid of eighths of [0, spread / 8) plus a jitter of a few float32 ulps..1e-3, so that many pairs share a corner and many
    IoUs sit at or next to a simple fraction (the thresholds 0.5 and 1 among them); scores on a grid of 1 / 16 (many ties) with every tenth jittered."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, spread, (n, b)) / 8.0
    l = rng.integers(0, spread, (n, b)) / 8.0
    h = rng.integers(1, 4, (n, b)) / 8.0
    w = rng.integers(1, 4, (n, b)) / 8.0
    jit = lambda: np.where(rng.random((n, b)) < 0.5, 0.0, rng.choice([1e-7, -1e-7, 1e-3, -1e-3], (n, b)))
    boxes = np.stack([t + jit(), l + jit(), t + h + jit(), l + w + jit()], axis=-1).astype(F)
    if repeat:  # the last `repeat` boxes of every image are copies of its first: pairs whose iou is exactly 1
        boxes[:, b - repeat:] = boxes[:, :repeat]
    scores = (rng.integers(0, 17, (n, c, b)) / 16.0).astype(F)
    scores = np.where(rng.random((n, c, b)) < 0.1, scores + rng.normal(0, 0.01, (n, c, b)).astype(F), scores).astype(F)
    return (to_center(boxes) if center else boxes), scores


def clustered(seed, b, clusters=3):
    """One image, one class, `b` boxes that are copies of `clusters` disjoint boxes in long runs, random scores: the selected list never holds more than
    `clusters` members however many candidates there are, and its members move forward as higher scores arrive."""
    rng = np.random.default_rng(seed)
    which = (np.arange(b) * clusters // b + (rng.random(b) < 0.02) * rng.integers(0, clusters, b)) % clusters
    base = np.array([[0, 4 * k, 1, 4 * k + 1] for k in range(clusters)], F)
    scores = rng.random((1, 1, b)).astype(F)
    scores[0, 0, 5] = 0.99999  # a member in the first word of `alive` that stays to the end
    return base[which][None], scores


SECOND_BLOCK_IOU = 0.3


def second_block():
    """One image, one class, every box a candidate (position == box index), iou threshold SECOND_BLOCK_IOU: a list whose members sit in words of `alive`
    at and past NMS_RESOLVE_THREADS (candidates from 65536 on: the second block of 64 words of a wave, whose removals travel through memory).
    Box 0 (score 0.99) and the filler (the same box, score 0.01: rejected by box 0 at once) keep the rule's loop short.  Groups live on rows of their own
    and never touch each other; a group is three disjoint boxes m1, m2, m3 side by side and X, which covers all three with a hull iou of 100 / 310.
      dense   word 1025 (wave 1) holds the 24 members of groups 1-8, scores (0.3, 0.2, 0.9)
      sparse  words 1024, 1040, 1056 (all wave 0) hold two members each: group 9's m1 (0.2), m2 (0.9); group 10's m1 (0.3), m2 (0.2); group 11's m1 (0.9), m3 (0.4)
    and from word 1058 on the probes: X of group 1 at 0.5 (removes m1 and m2, then blocked by m3 in the same dense word), X of group 2 at 0.95 (removes all
    three and joins), X of group 3 at 0.1 (blocked by m1), m2 of group 4 at 0.25 (removes it and joins), the two-box cover of group 9 at 0.5 (removes m1,
    blocked by m2 in the same sparse word), of group 10 at 0.95 (removes both and joins), m1 of group 11 at 0.5 (blocked), m3 of group 11 at 0.6 (removes
    it and joins), X of group 5 at 0.95 again after those (walks past the new members).  -> (boxes [1, B, 4], scores [1, 1, B])."""
    first = NMS_RESOLVE_THREADS * 64
    b = first + 64 * 34 + 20
    boxes = np.tile(np.array([500, 500, 510, 510], F), (b, 1))
    scores = np.full(b, 0.01, F)
    scores[0] = 0.99
    row = lambda g: 20.0 * g
    m = lambda g, k: [row(g), 10.5 * k, row(g) + 10, 10.5 * k + 10]
    cover = lambda g, k: [row(g), 0, row(g) + 10, 10.5 * (k - 1) + 10]   # covers m1 .. mk
    def put(pos, box, score):
        boxes[pos], scores[pos] = box, score
    at = first + 64  # word 1025
    for g in range(1, 9):
        for k, s in enumerate((0.3, 0.2, 0.9)):
            put(at, m(g, k), s)
            at += 1
    put(first, m(9, 0), 0.2); put(first + 1, m(9, 1), 0.9)                       # word 1024
    put(first + 64 * 16, m(10, 0), 0.3); put(first + 64 * 16 + 1, m(10, 1), 0.2)   # word 1040
    put(first + 64 * 32, m(11, 0), 0.9); put(first + 64 * 32 + 1, m(11, 2), 0.4)   # word 1056
    at = first + 64 * 34 + 3  # word 1058
    for box, s in ((cover(1, 3), 0.5), (cover(2, 3), 0.95), (cover(3, 3), 0.1), (m(4, 1), 0.25), (cover(9, 2), 0.5), (cover(10, 2), 0.95), (m(11, 0), 0.5),
                   (m(11, 2), 0.6), (cover(5, 3), 0.95)):
        put(at, box, s)
        at += 1
    assert at <= b
    return boxes[None], scores[None, None]
