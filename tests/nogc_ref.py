"""Plain-numpy restatement of the box evaluation's two extra groups of numbers: the
no-graph-constraint ranking / recalls (`SGRecall.calculate_recall`, sgg_metrics.py:254-343) and
the box IoU statistic (`_compute_iou_bbox`, :1133-1178).  Imports neither the product nor the
reference; the tests compare both against it.

Ties.  numpy's default sort leaves the order of equal scores unspecified, so the reference has
no answer there.  This file states the library's rule: inside a row and in the global ranking
the candidate with the smaller (r, c) wins (-0 == +0).  On tie-free scores it is the
reference's order.

Arithmetic.  The candidate score is (s_sub * s_obj) * rel_dists[r][c] in float32, two rounded
multiplications in that order (`obj_scores[pred_rel_inds].prod(1)[:, None] * rel_scores[:, 1:]`).
"""
from functools import reduce

import numpy as np

from oracle import evaluation as OE

TOP = 100          # `pred_to_gt[:100]` (:306-308)


def products(det_scores, rel_pairs, rel_dists):
    """[R][C1 - 1] float32 candidate scores."""
    s = np.asarray(det_scores, np.float32)
    rd = np.asarray(rel_dists, np.float32)
    rel_pairs = np.asarray(rel_pairs)
    pair = (s[rel_pairs[:, 0]] * s[rel_pairs[:, 1]]).astype(np.float32)
    out = pair[:, None] * rd[:, 1:]
    assert out.dtype == np.float32
    return out


def nogc_rank(det_scores, labels, rel_pairs, rel_dists, t, K=TOP):
    """The first min(K, R * t) of the ranking: dict(triplets [n][3], sub_rows [n], obj_rows [n],
    scores [n] float32, pred [n] (predicate), row [n] (pair index), count)."""
    labels, rel_pairs = np.asarray(labels), np.asarray(rel_pairs)
    prod = products(det_scores, rel_pairs, rel_dists)
    R, P1 = prod.shape
    assert 1 <= t <= P1
    # per-row cut: descending, ties -> smaller c (a stable sort of the negated scores)
    order = np.argsort(-prod, axis=1, kind="stable")
    keep = np.zeros((R, P1), bool)
    np.put_along_axis(keep, order[:, :t], True, axis=1)
    r, c0 = np.nonzero(keep)
    sc = prod[r, c0]
    flat = r * P1 + c0
    rank = np.lexsort((flat, -sc))            # primary: descending score; then smaller (r, c)
    rank = rank[:min(K, R * t)]
    r, c0, sc = r[rank], c0[rank], sc[rank]
    sub, obj = rel_pairs[r, 0], rel_pairs[r, 1]
    return dict(triplets=np.column_stack((labels[sub], c0 + 1, labels[obj])).astype(np.int64),
                sub_rows=sub.astype(np.int64), obj_rows=obj.astype(np.int64), scores=sc,
                pred=c0 + 1, row=r, count=int(rank.shape[0]))


def tie_free(det_scores, rel_pairs, rel_dists):
    """All R * (C1 - 1) products pairwise distinct (numpy's order is then determined)."""
    p = products(det_scores, rel_pairs, rel_dists).reshape(-1)
    return np.unique(p).shape[0] == p.shape[0]


def recall(pred_to_gt, num_gt, ks=(20, 50, 100)):
    out = {}
    for k in ks:
        match = reduce(np.union1d, pred_to_gt[:k], np.zeros(0, np.int64))
        out[k] = float(len(match)) / float(num_gt)
    return out


def evaluate_boxes_nogc(labels, rel_pairs, rel_dists, det, gt_rels, gt_labels, gt_boxes,
                        thresholds, thr=0.5, ks=(20, 50, 100)):
    """det [2R][5] (box, score).  Per threshold t: "nogc@t_pred_to_gt", "phrdet_nogc@t_pred_to_gt"
    (lists of min(100, R t) lists) and "nogc@t_recall", "phrdet_nogc@t_recall"."""
    det = np.asarray(det, np.float32)
    gt_rels, gt_labels = np.asarray(gt_rels), np.asarray(gt_labels)
    gt_boxes = np.asarray(gt_boxes, np.float32)
    gt_trip = np.column_stack((gt_labels[gt_rels[:, 0]], gt_rels[:, 2], gt_labels[gt_rels[:, 1]]))
    gt_tb = np.column_stack((gt_boxes[gt_rels[:, 0]], gt_boxes[gt_rels[:, 1]]))
    out = {}
    for t in thresholds:
        rk = nogc_rank(det[:, 4], labels, rel_pairs, rel_dists, t)
        p_tb = np.column_stack((det[rk["sub_rows"], :4], det[rk["obj_rows"], :4]))
        for pre, ph in (("", False), ("phrdet_", True)):
            lists = OE.pred_matches_bbox(gt_trip, rk["triplets"], gt_tb, p_tb, thr, phrdet=ph)
            out[pre + "nogc@%d_pred_to_gt" % t] = lists
            out[pre + "nogc@%d_recall" % t] = recall(lists, gt_rels.shape[0], ks)
    return out


def iou_bbox(gt_labels, pred_labels, gt_boxes, pred_boxes, R=None):
    """Two lists of float32 (subject side: predictions [0, R); object side: [R, 2R)), one entry
    per ground-truth object whose class that side predicts: the best IoU over those."""
    gt_labels, pred_labels = np.asarray(gt_labels), np.asarray(pred_labels)
    gt_boxes = np.asarray(gt_boxes, np.float32)
    pred_boxes = np.asarray(pred_boxes, np.float32)[:, :4]
    R = pred_labels.shape[0] // 2 if R is None else R
    out = []
    for lo in (0, R):
        cls, box = pred_labels[lo:lo + R], pred_boxes[lo:lo + R]
        vals = []
        for o in range(gt_labels.shape[0]):
            same = cls == gt_labels[o]
            if same.any():
                vals.append(max(OE.bbox_overlaps(gt_boxes[o][None], box[same]).numpy()[0]))
        out.append(vals)
    return out[0], out[1]


def dataset_numbers(per_image, gt_rels_list, num_rel, thresholds, ks=(20, 50, 100)):
    """The `nogc_result_dict` numbers over several images: {t: {"sgdet_recall": {k: mean},
    "sgdet_mean_recall": {k: .}, "sgdet_mean_recall_list": {k: [..]}, "phrdet_...": ...}} from
    the per-image dicts of `evaluate_boxes_nogc` (images without relations are left out by the
    caller, as the reference's loop does)."""
    out = {}
    for t in thresholds:
        out[t] = {}
        for mode, pre in (("sgdet", ""), ("phrdet", "phrdet_")):
            out[t][mode + "_recall"] = {
                k: float(np.mean([img[pre + "nogc@%d_recall" % t][k] for img in per_image]))
                for k in ks}
            coll = [OE.mean_recall_collect(img[pre + "nogc@%d_pred_to_gt" % t], g, num_rel, ks)
                    for img, g in zip(per_image, gt_rels_list)]
            mr, lst = OE.mean_recall(coll, num_rel, ks)
            out[t][mode + "_mean_recall"], out[t][mode + "_mean_recall_list"] = mr, lst
    return out
