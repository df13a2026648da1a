"""Device-side feed of the PSG evaluator (consumer side).

The reference's `SGRecall.calculate_recall` (pairnet/evaluation/sgg_metrics.py:173-252)
takes a `Result` on the host: it forms the predicted triplets (:207-209, :1292-1308),
matches them with the ground-truth triplets by class equality and mask IoU >= 0.5
(`_compute_pred_matches_panseg`, :1311-1371, `mask_iou` :1374-1380: a Python loop of
`np.count_nonzero` over full-size masks) and counts recall@K over the triplets in query
order (:95-99).  `TripletEvaluator` produces the same `pred_to_gt` lists and recalls from
the device-resident 8-tuple of `get_bboxes`, so the 200 full-size masks never leave the
GPU: masks are bit-packed (`pn_pack_mask_bits`), the IoU counts are exact integer popcounts
(`pn_mask_iou_counts`), the match matrix is one small kernel (`pn_triplet_match`); only
that R x G byte matrix is copied to the host.  `SceneGraphMetrics` is the dataset-level
aggregation on top: R@K averaged over images (:100-141), the reference's headline metric
mean recall (`SGMeanRecall`, :669-916: per-predicate recall averaged over the images that
have the predicate, then over the predicates), phrase-detection variants, and the
subject / object IoU statistic (`_compute_iou_panseg`, :1087-1131, from the same exact
popcounts).  Images without ground-truth relations are skipped, as the reference's
`sgg_evaluate` loop does.

Box results (`detection_method="bbox"`) get what the reference adds for them: the
no-graph-constraint recalls (:254-343; `nogc=`, ranked on the device by csrc/nogc.hip) and the
box IoU statistic (`_compute_iou_bbox`, :1133-1178; `iou=`), on `evaluate_boxes`,
`SceneGraphMetrics` and `StreamingEvaluator.add_boxes`; both are off by default.

`PanopticQuality` is the reference's other metric, `--eval PQ` (pairnet/datasets/psg.py:309-335):
PQ / SQ / RQ of the panoptic maps, from a per-image record csrc/panoptic_quality.hip leaves on
the device.
"""
import numpy as np
import torch

from . import hip


def _tensor(x):
    """Ground truth as handed in: numpy, lists, or tensors (host or ALREADY on the device, as
    `pairnet_amd.dataset.eval_ground_truth` leaves the masks)."""
    return x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))


NOGC_TOP = 100      # the reference counts only the best 100 no-graph-constraint triplets
#                     (`pred_to_gt[:100]`, sgg_metrics.py:306-308, :314, :333, :339)


def nogc_thresholds(nogc, num_predicates, ks):
    """The `nogc` keyword as a tuple of thresholds (the reference's `nogc_thres_num`): None ->
    (), True -> the reference's default `(num_predicates,)` (sgg_eval.py:74-75), an int or up to
    4 distinct ints in [1, num_predicates].  The reference truncates the ranked list at 100
    whatever k is; here a k above 100 is refused instead of being truncated quietly."""
    if nogc is None or nogc is False:
        return ()
    if nogc is True:
        ts = (int(num_predicates),)
    elif isinstance(nogc, (int, np.integer)):
        ts = (int(nogc),)
    else:
        ts = tuple(int(t) for t in nogc)
    if not 1 <= len(ts) <= 4 or len(set(ts)) != len(ts):
        raise ValueError("nogc: 1..4 distinct thresholds, got %r" % (ts,))
    if min(ts) < 1 or max(ts) > int(num_predicates):
        raise ValueError("nogc: thresholds must lie in [1, %d], got %r" % (num_predicates, ts))
    if any(int(k) > NOGC_TOP for k in ks):
        raise ValueError("nogc: only the best %d triplets are ranked (sgg_metrics.py:306-308); "
                         "k = %r is not served" % (NOGC_TOP, tuple(ks)))
    return ts


class TripletEvaluator:
    def __init__(self, iou_thr=0.5, ks=(20, 50, 100)):
        self.iou_thr, self.ks = float(iou_thr), tuple(ks)

    @torch.no_grad()
    @hip.on_device
    def match(self, result, gt_rels, gt_labels, gt_masks, phrdet=False, ignore_rel=False):
        """result: the 8-tuple of `get_bboxes` (device tensors); gt_rels (G, 3) int
        (sub_id, obj_id, predicate); gt_labels (n_obj,) int; gt_masks (n_obj, H, W) bool,
        at the masks' resolution.  Returns the uint8 match matrix [R][G] on the device."""
        labels, masks, r_dists = result[1], result[3], result[7]
        dev = masks.device
        R, C1 = r_dists.shape
        H, W = masks.shape[-2:]
        gt_rels = _tensor(gt_rels).cpu().to(torch.int64)
        gt_labels = _tensor(gt_labels).cpu().to(torch.int64)
        G, nobj = int(gt_rels.shape[0]), int(gt_labels.shape[0])
        gt_masks = _tensor(gt_masks).to(dev).view(nobj, H, W)
        i32 = lambda t: t.to(torch.int32).to(dev).contiguous()
        gtrip = i32(torch.stack([gt_labels[gt_rels[:, 0]], gt_rels[:, 2],
                                 gt_labels[gt_rels[:, 1]]], 1))
        ptrip = torch.empty(R, 3, device=dev, dtype=torch.int32)
        score = torch.empty(R, device=dev, dtype=torch.float32)
        hip.pred_triplets(labels, r_dists, ptrip, score, R, C1)
        nw = (H * W + 63) // 64
        pw = torch.empty(2 * R, nw, device=dev, dtype=torch.int64)
        gw = torch.empty(nobj, nw, device=dev, dtype=torch.int64)
        hip.pack_mask_bits(masks.view(torch.uint8), pw, 2 * R, H * W)
        hip.pack_mask_bits(gt_masks.to(torch.uint8), gw, nobj, H * W)
        ar = torch.arange(R, dtype=torch.int32, device=dev)
        ps, po = ar, ar + R                              # rel_pairs[r] = (r, R + r)
        gs, go = i32(gt_rels[:, 0]), i32(gt_rels[:, 1])
        if phrdet:                                       # union masks (:1343-1350)
            pu = torch.empty(R, nw, device=dev, dtype=torch.int64)
            gu = torch.empty(G, nw, device=dev, dtype=torch.int64)
            hip.mask_or_rows(pw, ps, po, pu, R, nw)
            hip.mask_or_rows(gw, gs, go, gu, G, nw)
            pw, gw, np_, ng = pu, gu, R, G
            ps, gs = ar, torch.arange(G, dtype=torch.int32, device=dev)
            po = go = None
        else:
            np_, ng = 2 * R, nobj
        inter = torch.empty(np_, ng, device=dev, dtype=torch.int32)
        ap = torch.empty(np_, device=dev, dtype=torch.int32)
        ag = torch.empty(ng, device=dev, dtype=torch.int32)
        hip.mask_iou_counts(pw, np_, gw, ng, nw, inter, ap, ag)
        match = torch.empty(R, G, device=dev, dtype=torch.uint8)
        hip.triplet_match(ptrip, gtrip, R, G, inter, ap, ag, ng, ps, po, gs, go, self.iou_thr,
                          phrdet, ignore_rel, match)
        return match

    @torch.no_grad()
    @hip.on_device
    def match_boxes(self, result, gt_rels, gt_labels, gt_boxes, phrdet=False, ignore_rel=False):
        """`detection_method="bbox"`: result = the 6-tuple of `CrossHeadBBox.get_bboxes`
        (det_bboxes [2R,5], labels, rel_pairs, ., ., r_dists); gt_boxes (n_obj, 4) xyxy.
        `_compute_pred_matches_bbox` (sgg_metrics.py:1212-1273) on the device; returns the uint8
        match matrix [R][G]."""
        det, labels, r_dists = result[0], result[1], result[5]
        dev = det.device
        R, C1 = r_dists.shape
        G, gtrip, gs, go, gbox = self._box_ground_truth(gt_rels, gt_labels, gt_boxes, dev)
        ptrip = torch.empty(R, 3, device=dev, dtype=torch.int32)
        score = torch.empty(R, device=dev, dtype=torch.float32)
        hip.pred_triplets(labels, r_dists, ptrip, score, R, C1)
        ar = torch.arange(R, dtype=torch.int32, device=dev)
        match = torch.empty(R, G, device=dev, dtype=torch.uint8)
        hip.triplet_match_boxes(ptrip, gtrip, R, G, det, det.stride(0), gbox, 4, ar, ar + R,
                                gs, go, self.iou_thr, phrdet, ignore_rel, match)
        return match

    @staticmethod
    def _box_ground_truth(gt_rels, gt_labels, gt_boxes, dev):
        """(G, gt triplets [G][3], subject rows [G], object rows [G] int32, boxes [n_obj][4]
        float32) on the device."""
        gt_rels = _tensor(gt_rels).cpu().to(torch.int64)
        gt_labels = _tensor(gt_labels).cpu().to(torch.int64)
        gbox = torch.as_tensor(np.asarray(gt_boxes), dtype=torch.float32).to(dev).contiguous()
        i32 = lambda t: t.to(torch.int32).to(dev).contiguous()
        gtrip = i32(torch.stack([gt_labels[gt_rels[:, 0]], gt_rels[:, 2],
                                 gt_labels[gt_rels[:, 1]]], 1))
        return int(gt_rels.shape[0]), gtrip, i32(gt_rels[:, 0]), i32(gt_rels[:, 1]), gbox

    @torch.no_grad()
    @hip.on_device
    def match_boxes_nogc(self, result, gt_rels, gt_labels, gt_boxes, per_row):
        """The no-graph-constraint part of `calculate_recall` (sgg_metrics.py:254-343) for one
        threshold `per_row` (the reference's `nogc_num`): the best `NOGC_TOP` of the R x
        `per_row` surviving (pair, predicate) candidates, ranked on the device
        (`pn_nogc_triplets_f32`) and matched as sgdet and as phrdet.  Returns the two uint8 match
        matrices [P][G], P = min(NOGC_TOP, R * per_row)."""
        det, labels, r_dists = result[0], result[1], result[5]
        dev = det.device
        R, C1 = r_dists.shape
        G, gtrip, gs, go, gbox = self._box_ground_truth(gt_rels, gt_labels, gt_boxes, dev)
        K = NOGC_TOP
        P = min(K, R * int(per_row))
        e32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
        trip, srow, orow, count = e32(K, 3), e32(K), e32(K), e32(1)
        score = torch.empty(K, device=dev, dtype=torch.float32)
        ar = torch.arange(R, dtype=torch.int32, device=dev)      # rel_pairs[r] = (r, R + r)
        hip.nogc_triplets(det, det.stride(0), labels, r_dists.contiguous(), ar, ar + R, R, C1,
                          int(per_row), K, trip, srow, orow, score, count)
        out = []
        for ph in (False, True):
            match = torch.empty(P, G, device=dev, dtype=torch.uint8)
            hip.triplet_match_boxes(trip, gtrip, P, G, det, det.stride(0), gbox, 4, srow, orow,
                                    gs, go, self.iou_thr, ph, False, match)
            out.append(match)
        return out[0], out[1]

    @torch.no_grad()
    @hip.on_device
    def iou_stats_boxes(self, result, gt_labels, gt_boxes):
        """`SGObjectIOU.calculate_iou` -> `_compute_iou_bbox` (sgg_metrics.py:1025-1028,
        :1133-1178): for every ground-truth OBJECT whose class occurs among the subject (object)
        predictions, the best box IoU over the predictions of that class.  Returns two float64
        arrays (subjects, objects), in ground-truth object order, each the exact value of the
        reference's float32."""
        det, labels = result[0], result[1]
        dev = det.device
        R = int(labels.shape[0]) // 2
        lab = torch.as_tensor(np.asarray(gt_labels)).reshape(-1).to(torch.int32).to(dev)
        nobj = int(lab.shape[0])
        if nobj == 0:
            return np.zeros(0), np.zeros(0)
        gbox = torch.as_tensor(np.asarray(gt_boxes), dtype=torch.float32).reshape(nobj, 4)
        gbox = gbox.to(dev).contiguous()
        valid = torch.empty(2 * nobj, device=dev, dtype=torch.uint8)
        best = torch.empty(2 * nobj, device=dev, dtype=torch.float64)
        hip.eval_iou_best_boxes(det, det.stride(0), labels, R, gbox, 4, lab, nobj, valid, best)
        valid, best = valid.cpu().numpy().astype(bool), best.cpu().numpy()
        return best[:nobj][valid[:nobj]], best[nobj:][valid[nobj:]]

    def evaluate_boxes(self, result, gt_rels, gt_labels, gt_boxes, nogc=None, iou=False):
        """sgdet + phrdet recalls of one image from box results (`calculate_recall`,
        sgg_metrics.py:173-252).  `nogc` (see `nogc_thresholds`) adds the no-graph-constraint
        part (:254-343), per threshold t the reference's `local_container` keys
        "nogc@t_pred_to_gt" / "phrdet_nogc@t_pred_to_gt" (lists of at most 100 lists) and
        "nogc@t_recall" / "phrdet_nogc@t_recall"; `iou=True` adds "sub_iou" / "obj_iou"
        (`iou_stats_boxes`).  The reference's "..._all_pred_to_gt" and "..._pred_pair_in_gt"
        entries feed only `SGPairAccuracy`, which does nothing in sgdet mode: left out."""
        n = len(gt_rels)
        R, C1 = (int(v) for v in result[5].shape)
        ts = nogc_thresholds(nogc, C1 - 1, self.ks)
        if n == 0:
            out = dict(pred_to_gt=[[] for _ in range(R)], phrdet_pred_to_gt=[[] for _ in range(R)],
                       sgdet_recall=None, phrdet_recall=None)
            for t in ts:
                for pre in ("", "phrdet_"):
                    out[pre + "nogc@%d_pred_to_gt" % t] = [[] for _ in range(min(NOGC_TOP, R * t))]
                    out[pre + "nogc@%d_recall" % t] = None
            return out
        p2g = self.pred_to_gt(self.match_boxes(result, gt_rels, gt_labels, gt_boxes))
        ph = self.pred_to_gt(self.match_boxes(result, gt_rels, gt_labels, gt_boxes, phrdet=True))
        out = dict(pred_to_gt=p2g, phrdet_pred_to_gt=ph, sgdet_recall=self.recall(p2g, n),
                   phrdet_recall=self.recall(ph, n))
        for t in ts:
            ms = self.match_boxes_nogc(result, gt_rels, gt_labels, gt_boxes, t)
            for pre, m in zip(("", "phrdet_"), ms):
                lists = self.pred_to_gt(m)
                out[pre + "nogc@%d_pred_to_gt" % t] = lists
                out[pre + "nogc@%d_recall" % t] = self.recall(lists, n)
        if iou:
            out["sub_iou"], out["obj_iou"] = self.iou_stats_boxes(result, gt_labels, gt_boxes)
        return out

    def pred_to_gt(self, match):
        """The reference's list of lists (one D2H copy of R x G bytes)."""
        m = match.cpu().numpy().astype(bool)
        return [np.nonzero(row)[0].tolist() for row in m]

    def recall(self, pred_to_gt, num_gt):
        """recall@K over the triplets in query (= top-k) order (:95-99)."""
        out = {}
        for k in self.ks:
            hit = set()
            for lst in pred_to_gt[:k]:
                hit.update(lst)
            out[k] = len(hit) / float(num_gt)
        return out

    @torch.no_grad()
    @hip.on_device
    def iou_stats(self, result, gt_rels, gt_labels, gt_masks):
        """`_compute_iou_panseg` (sgg_metrics.py:1087-1131) from device-resident masks: for
        every ground-truth triplet whose subject (object) class occurs among the 2R predicted
        labels, the best mask IoU over the predictions of that class.  Returns two float64
        arrays (subjects, objects), in ground-truth triplet order."""
        labels, masks = result[1], result[3]
        dev = masks.device
        H, W = masks.shape[-2:]
        gt_rels = np.asarray(gt_rels)
        gt_labels_np = np.asarray(gt_labels)
        nobj, P = int(gt_labels_np.shape[0]), int(masks.shape[0])
        gm = _tensor(gt_masks).to(dev).view(nobj, H, W)
        nw = (H * W + 63) // 64
        pw = torch.empty(P, nw, device=dev, dtype=torch.int64)
        gw = torch.empty(nobj, nw, device=dev, dtype=torch.int64)
        hip.pack_mask_bits(masks.view(torch.uint8), pw, P, H * W)
        hip.pack_mask_bits(gm.to(torch.uint8), gw, nobj, H * W)
        inter = torch.empty(P, nobj, device=dev, dtype=torch.int32)
        ap = torch.empty(P, device=dev, dtype=torch.int32)
        ag = torch.empty(nobj, device=dev, dtype=torch.int32)
        hip.mask_iou_counts(pw, P, gw, nobj, nw, inter, ap, ag)
        inter, ap, ag = (t.cpu().numpy().astype(np.int64) for t in (inter, ap, ag))
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = inter.astype(np.float64) / (ap[:, None] + ag[None, :] - inter).astype(np.float64)
        pl = labels.cpu().numpy()
        out = []
        for col in (0, 1):
            vals = []
            for g in range(gt_rels.shape[0]):
                o = int(gt_rels[g, col])
                same = pl == gt_labels_np[o]
                if same.any():
                    best = 0
                    for v in iou[same, o]:      # (python max(v, best) with the reference's argument
                        # order: a NaN IoU -- empty prediction AND empty ground truth -- DOES
                        # replace `best`, max(nan, x) returns nan; kept for parity)
                        best = max(v, best)
                    vals.append(best)
            out.append(np.array(vals))
        return out[0], out[1]

    def __call__(self, result, gt_rels, gt_labels, gt_masks):
        """sgdet + phrdet recalls of one image, as `calculate_recall` records them.  An image
        without ground-truth relations has nothing to match (the reference's loop skips it):
        empty lists, no recalls."""
        n = len(gt_rels)
        if n == 0:
            R = int(result[7].shape[0])
            return dict(pred_to_gt=[[] for _ in range(R)], phrdet_pred_to_gt=[[] for _ in range(R)],
                        sgdet_recall=None, phrdet_recall=None)
        p2g = self.pred_to_gt(self.match(result, gt_rels, gt_labels, gt_masks))
        ph = self.pred_to_gt(self.match(result, gt_rels, gt_labels, gt_masks, phrdet=True))
        return dict(pred_to_gt=p2g, phrdet_pred_to_gt=ph, sgdet_recall=self.recall(p2g, n),
                    phrdet_recall=self.recall(ph, n))


class SceneGraphMetrics:
    """Dataset-level aggregation of `TripletEvaluator` outputs: what the reference's
    `sgg_evaluate` prints for mode "sgdet" -- R@K and mR@K (graph constraint), their
    phrase-detection variants, and the subject / object IoU lists.

        metrics = SceneGraphMetrics(num_predicates=56)
        for each image:  metrics.add(evaluator(result, gt_rels, gt_labels, gt_masks), gt_rels)
        metrics.summary()   ->  {"sgdet_recall": {20: .., 50: .., 100: ..},
                                 "sgdet_mean_recall": {...}, "sgdet_mean_recall_list": {...},
                                 "phrdet_recall": ..., "phrdet_mean_recall": ..., "images": n}
    """

    def __init__(self, num_predicates, ks=(20, 50, 100), nogc=None):
        self.num_rel = int(num_predicates) + 1        # + __background__ (:681-683)
        self.ks = tuple(ks)
        self.recalls = {m: {k: [] for k in self.ks} for m in ("sgdet", "phrdet")}
        self.collect = {m: {k: [[] for _ in range(self.num_rel)] for k in self.ks}
                        for m in ("sgdet", "phrdet")}
        # the reference's `nogc_result_dict` (:69-79, :698-735): the same two containers once
        # per no-graph-constraint threshold (box results only)
        self.nogc = nogc_thresholds(nogc, int(num_predicates), self.ks)
        self.nogc_recalls = {t: {m: {k: [] for k in self.ks} for m in ("sgdet", "phrdet")}
                             for t in self.nogc}
        self.nogc_collect = {t: {m: {k: [[] for _ in range(self.num_rel)] for k in self.ks}
                                 for m in ("sgdet", "phrdet")} for t in self.nogc}
        self.sub_iou, self.obj_iou = [], []
        self.images = self.skipped = 0

    def _collect(self, mode, pred_to_gt, gt_rels, target=None):
        """`SGMeanRecall._collect_single` (:741-766); `target`: the container of one
        no-graph-constraint threshold instead of the graph-constrained one."""
        collect = self.collect if target is None else target
        for k in self.ks:
            match = set()
            for lst in pred_to_gt[:k]:
                match.update(lst)
            hit, count = [0] * self.num_rel, [0] * self.num_rel
            for g in range(gt_rels.shape[0]):
                count[int(gt_rels[g, 2])] += 1
                count[0] += 1
            for g in match:
                hit[int(gt_rels[int(g), 2])] += 1
                hit[0] += 1
            for n in range(self.num_rel):
                if count[n] > 0:
                    collect[mode][k][n].append(float(hit[n] / count[n]))

    def add(self, image_eval, gt_rels, iou=None):
        """`image_eval`: what `TripletEvaluator.__call__` / `evaluate_boxes` returned for the
        image (with `nogc` set: `evaluate_boxes(..., nogc=...)` with at least these thresholds);
        `iou`: optionally `TripletEvaluator.iou_stats(...)` of the same image (default: the
        "sub_iou" / "obj_iou" entries `evaluate_boxes(..., iou=True)` left, if any)."""
        gt_rels = np.asarray(gt_rels).reshape(-1, 3)
        if gt_rels.shape[0] == 0:
            self.skipped += 1
            return
        self.images += 1
        for mode, key in (("sgdet", "pred_to_gt"), ("phrdet", "phrdet_pred_to_gt")):
            for k in self.ks:
                self.recalls[mode][k].append(image_eval[mode + "_recall"][k])
            self._collect(mode, image_eval[key], gt_rels)
        for t in self.nogc:                       # (:312-319, :337-343, :882-899)
            for mode, pre in (("sgdet", ""), ("phrdet", "phrdet_")):
                for k in self.ks:
                    self.nogc_recalls[t][mode][k].append(image_eval[pre + "nogc@%d_recall" % t][k])
                self._collect(mode, image_eval[pre + "nogc@%d_pred_to_gt" % t], gt_rels,
                              target=self.nogc_collect[t])
        if iou is None and "sub_iou" in image_eval:
            iou = (image_eval["sub_iou"], image_eval["obj_iou"])
        if iou is not None:
            self.sub_iou.extend(iou[0])
            self.obj_iou.extend(iou[1])

    def summary(self):
        """`SGRecall._print_single` / `SGMeanRecall._calculate_single` (:768-792)."""
        out = dict(images=self.images, skipped=self.skipped)

        def fill(dst, recalls, collect):
            for mode in ("sgdet", "phrdet"):
                dst[mode + "_recall"] = {k: float(np.mean(v)) if v else 0.0
                                         for k, v in recalls[mode].items()}
                mr, lists = {}, {}
                for k in self.ks:
                    per = collect[mode][k]
                    lst = [0.0 if len(per[n + 1]) == 0 else float(np.mean(per[n + 1]))
                           for n in range(self.num_rel - 1)]
                    lists[k] = lst
                    mr[k] = sum(lst) / float(self.num_rel - 1)
                dst[mode + "_mean_recall"], dst[mode + "_mean_recall_list"] = mr, lists

        fill(out, self.recalls, self.collect)
        if self.nogc:                             # the reference's `nogc_result_dict`
            out["nogc"] = {}
            for t in self.nogc:
                out["nogc"][t] = {}
                fill(out["nogc"][t], self.nogc_recalls[t], self.nogc_collect[t])
        if self.sub_iou or self.obj_iou:
            out["subject-IoU"] = float(np.mean(self.sub_iou)) if self.sub_iou else 0.0
            out["object-IoU"] = float(np.mean(self.obj_iou)) if self.obj_iou else 0.0
        return out

    @staticmethod
    def pred_pair_in_gt(rel_pairs, gt_rels):
        """`SGPairAccuracy.prepare_gtpair` (:632-641).  (The accuracy itself is only
        accumulated for modes other than "sgdet", :571-585: nothing to add for PSG.)"""
        rel_pairs, gt_rels = np.asarray(rel_pairs), np.asarray(gt_rels)
        p = rel_pairs[:, 0] * 10000 + rel_pairs[:, 1]
        g = gt_rels[:, 0] * 10000 + gt_rels[:, 1]
        return (p[:, None] == g[None, :]).sum(-1) > 0


def host_record(image_eval, gt_rels, num_rel, ks=(20, 50, 100), nogc=None):
    """One image's recall record in numpy, from the `pred_to_gt` lists `TripletEvaluator`
    returned: (hits [2][len(ks)][num_rel], counts [num_rel]) int32 -- what `pn_eval_record`
    leaves on the device (`reduce(np.union1d, pred_to_gt[:k])`, sgg_metrics.py:95-99, fed
    through `_collect_single`, :741-766; slot 0 counts every predicate).  With `nogc` (a tuple
    of thresholds) a third array follows: nogc_hits [len(nogc)][2][len(ks)][num_rel], the same
    counts from the "nogc@t_pred_to_gt" / "phrdet_nogc@t_pred_to_gt" lists."""
    gt_rels = np.asarray(gt_rels).reshape(-1, 3)
    pred = gt_rels[:, 2].astype(np.int64)
    counts = np.zeros(num_rel, np.int32)
    np.add.at(counts, pred, 1)
    counts[0] = gt_rels.shape[0]

    def hits_of(keys):
        hits = np.zeros((2, len(ks), num_rel), np.int32)
        for m, key in enumerate(keys):
            for j, k in enumerate(ks):
                lists = image_eval[key][:k]
                match = np.unique(np.concatenate([np.asarray(l, np.int64) for l in lists]
                                                 + [np.zeros(0, np.int64)]))
                np.add.at(hits[m, j], pred[match], 1)
                hits[m, j, 0] = match.shape[0]
        return hits

    hits = hits_of(("pred_to_gt", "phrdet_pred_to_gt"))
    if not nogc:
        return hits, counts
    more = [hits_of(("nogc@%d_pred_to_gt" % t, "phrdet_nogc@%d_pred_to_gt" % t)) for t in nogc]
    return hits, counts, np.stack(more)


class StreamingEvaluator:
    """`TripletEvaluator` + `SceneGraphMetrics` for a loop that must not wait for the GPU:
    `add()` enqueues one image's matching on the current stream and leaves a small integer
    record on the device (`pn_eval_record`: per k and predicate the number of ground-truth
    relations hit; `pn_eval_iou_best`: the subject / object IoU statistic as float64); nothing
    is read back before `state()` / `summary()`.  The summary equals
    `SceneGraphMetrics.summary()` of the host path bit for bit: only integers and IEEE float64
    quotients come from the device, and the host applies the reference's own float
    expressions to them in dataset order.

        ev = StreamingEvaluator(num_predicates=56)
        for each image i:  ev.add(result, gt_rels, gt_labels, gt_masks, index=i)
        ev.summary()

    Several ranks: `ev.merge(all ranks' ev.state())` on rank 0, then `ev.summary()`.
    Per-image `pred_to_gt` lists are not produced; `TripletEvaluator` stays for those.

    Box results: `ev.add_boxes(result, gt_rels, gt_labels, gt_boxes, index=i, iou=True)`; an
    evaluator built with `nogc=` also records the no-graph-constraint ranking per threshold
    (`summary()["nogc"]`), and then takes box results only."""

    _MAGIC = 0x5345                              # first word of a state blob
    _MAGIC_NOGC = 0x534E                         # ... of one that carries nogc thresholds

    def __init__(self, num_predicates, ks=(20, 50, 100), iou_thr=0.5, nogc=None):
        """`nogc` (see `nogc_thresholds`; box results only): `add_boxes` also leaves, per
        threshold, the record of the no-graph-constraint ranking (sgg_metrics.py:254-343), and
        `summary()` gains the `"nogc"` entry of `SceneGraphMetrics`."""
        self.num_predicates = int(num_predicates)
        self.num_rel = self.num_predicates + 1   # + __background__ (:681-683)
        self.ks = tuple(int(k) for k in ks)
        self.iou_thr = float(iou_thr)
        if not 1 <= len(self.ks) <= 8 or not 2 <= self.num_rel <= 256:
            raise ValueError("StreamingEvaluator: 1..8 values of k and at most 255 predicates")
        self.nogc = nogc_thresholds(nogc, self.num_predicates, self.ks)
        # ints per image: [hits 2 nk num_rel | counts num_rel | per threshold: hits 2 nk num_rel]
        self._nhits = 2 * len(self.ks) * self.num_rel
        self._nints = self._nhits + self.num_rel + len(self.nogc) * self._nhits
        self._host = {}       # index -> (G, ints [_nints] int32, sub f64, obj f64)
        self._skipped = set()
        self._dev = []        # (index, G, record, valid, best, event, IoU rows): not read back yet
        self._seen = set()    # every index added so far
        self._calls = 0

    def _config(self):
        """(magic, the header words behind [magic, images, skipped]): without `nogc` today's
        (nk, num_rel); with it another magic and the thresholds appended."""
        if not self.nogc:
            return self._MAGIC, [len(self.ks), self.num_rel]
        return self._MAGIC_NOGC, [len(self.ks), self.num_rel, len(self.nogc)] + list(self.nogc)

    # ---- ground truth: checked on the host, one pinned buffer, one non-blocking copy ----
    def _tables(self, gt_rels, gt_labels):
        if torch.is_tensor(gt_rels) and gt_rels.is_cuda or \
                torch.is_tensor(gt_labels) and gt_labels.is_cuda:
            raise ValueError("gt_rels / gt_labels are host data (only the masks live on the device)")
        rels = np.asarray(gt_rels).reshape(-1, 3).astype(np.int64)
        lab = np.asarray(gt_labels).reshape(-1).astype(np.int64)
        G, nobj = rels.shape[0], lab.shape[0]
        if G and (rels[:, 2].min() < 1 or rels[:, 2].max() >= self.num_rel):
            raise ValueError("gt_rels: predicate ids must lie in [1, %d)" % self.num_rel)
        if G and (rels[:, :2].min() < 0 or rels[:, :2].max() >= nobj):
            raise IndexError("gt_rels: subject / object rows must lie in [0, %d)" % nobj)
        return rels, lab, G, nobj

    def _upload(self, rels, lab, R, dev, extra=None):
        """[gt triplets 3G | subject rows G | object rows G | predicates G | labels n_obj |
        0..max(2R, G) | ks | extra] int32 -> device (the `_to_dev` idiom of losses.py)."""
        G = rels.shape[0]
        pieces = [np.stack([lab[rels[:, 0]], rels[:, 2], lab[rels[:, 1]]], 1).reshape(-1),
                  rels[:, 0], rels[:, 1], rels[:, 2], lab, np.arange(max(2 * R, G)),
                  np.asarray(self.ks)]
        pieces = [p.astype(np.int32) for p in pieces] + ([extra] if extra is not None else [])
        host = torch.from_numpy(np.concatenate(pieces))
        buf = torch.empty(host.shape[0], dtype=torch.int32, pin_memory=True)
        buf.copy_(host)
        up = buf.to(dev, non_blocking=True)
        out, o = [], 0
        for p in pieces:
            out.append(up[o:o + p.shape[0]])
            o += p.shape[0]
        return out

    def _index(self, index):
        idx = self._calls if index is None else int(index)
        self._calls += 1
        if idx in self._seen:
            raise ValueError("StreamingEvaluator: image %d was added before" % idx)
        self._seen.add(idx)
        return idx

    def _log(self, idx, G, rec, valid, best, iou_rows=None):
        """`iou_rows`: rows per side of valid / best (G on the mask path: one per relation;
        n_obj on the box path: one per object)."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(rec.device))
        self._dev.append((idx, G, rec, valid, best, ev, G if iou_rows is None else iou_rows))

    def _record(self, m_s, m_p, R, G, gpred, ks, dev):
        nk = len(self.ks)
        rec = torch.empty(self._nints, device=dev, dtype=torch.int32)
        hip.eval_record(m_s, m_p, R, G, gpred, ks, nk, self.num_rel,
                        rec[:self._nhits], rec[self._nhits:self._nhits + self.num_rel])
        return rec

    @torch.no_grad()
    @hip.on_device
    def add(self, result, gt_rels, gt_labels, gt_masks, index=None, iou=True):
        """result: the 8-tuple of `get_bboxes` (device tensors); gt_rels (G, 3) / gt_labels
        (n_obj,) host data; gt_masks (n_obj, H, W) bool, on the device as
        `dataset.eval_ground_truth` leaves them (host masks go up non-blocking).  Everything is
        enqueued on the current stream; nothing is read back."""
        if self.nogc:
            raise NotImplementedError(
                "StreamingEvaluator.add: no-graph-constraint recalls exist for box results only "
                "(the reference computes none for detection_method == \"pan_seg\", "
                "sgg_metrics.py:254); use add_boxes, or an evaluator without nogc")
        labels, masks, r_dists = result[1], result[3], result[7]
        dev = masks.device
        R, C1 = r_dists.shape
        rels, lab, G, nobj = self._tables(gt_rels, gt_labels)
        idx = self._index(index)
        if G == 0:                                # (the reference's loop skips the image)
            self._skipped.add(idx)
            return
        H, W = masks.shape[-2:]
        gtrip, gs, go, gpred, glab, ar, ks = self._upload(rels, lab, R, dev)
        gm = _tensor(gt_masks)
        if not gm.is_cuda:
            gm = gm.contiguous().pin_memory().to(dev, non_blocking=True)
        gm = gm.contiguous().view(nobj, H, W)
        gm = gm.view(torch.uint8) if gm.dtype == torch.bool else gm.to(torch.uint8)
        pm = masks.contiguous()
        pm = pm.view(torch.uint8) if pm.dtype == torch.bool else pm.to(torch.uint8)
        i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
        i64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int64)
        ptrip = i32(R, 3)
        score = torch.empty(R, device=dev, dtype=torch.float32)
        hip.pred_triplets(labels, r_dists, ptrip, score, R, C1)
        # both mask sets packed ONCE; one [2R, n_obj] count matrix for the sgdet match and the
        # IoU statistic; one union pass and one [R, G] count matrix for phrase detection
        nw = (H * W + 63) // 64
        pw, gw = i64(2 * R, nw), i64(nobj, nw)
        hip.pack_mask_bits(pm, pw, 2 * R, H * W)
        hip.pack_mask_bits(gm, gw, nobj, H * W)
        inter, ap, ag = i32(2 * R, nobj), i32(2 * R), i32(nobj)
        hip.mask_iou_counts(pw, 2 * R, gw, nobj, nw, inter, ap, ag)
        pu, gu = i64(R, nw), i64(G, nw)
        hip.mask_or_rows(pw, ar[:R], ar[R:2 * R], pu, R, nw)
        hip.mask_or_rows(gw, gs, go, gu, G, nw)
        inter_u, apu, agu = i32(R, G), i32(R), i32(G)
        hip.mask_iou_counts(pu, R, gu, G, nw, inter_u, apu, agu)
        m_s = torch.empty(R, G, device=dev, dtype=torch.uint8)
        m_p = torch.empty(R, G, device=dev, dtype=torch.uint8)
        hip.triplet_match(ptrip, gtrip, R, G, inter, ap, ag, nobj, ar[:R], ar[R:2 * R], gs, go,
                          self.iou_thr, False, False, m_s)
        hip.triplet_match(ptrip, gtrip, R, G, inter_u, apu, agu, G, ar[:R], None, ar[:G], None,
                          self.iou_thr, True, False, m_p)
        rec = self._record(m_s, m_p, R, G, gpred, ks, dev)
        valid = best = None
        if iou:
            valid = torch.empty(2 * G, device=dev, dtype=torch.uint8)
            best = torch.empty(2 * G, device=dev, dtype=torch.float64)
            hip.eval_iou_best(inter, ap, ag, 2 * R, nobj, labels, glab, gs, go, G, valid, best)
        self._log(idx, G, rec, valid, best)

    @torch.no_grad()
    @hip.on_device
    def add_boxes(self, result, gt_rels, gt_labels, gt_boxes, index=None, iou=False):
        """`detection_method="bbox"`: result = the 6-tuple of `CrossHeadBBox.get_bboxes`;
        gt_boxes (n_obj, 4) xyxy host data.  With `nogc` set, per threshold one ranking
        (`pn_nogc_triplets_f32`), two matches and one `pn_eval_record` more; `iou=True` also
        enqueues the box IoU statistic (`pn_eval_iou_best_boxes`: one row per ground-truth
        OBJECT).  Everything goes to the current stream; nothing is read back."""
        det, labels, r_dists = result[0], result[1], result[5]
        dev = det.device
        R, C1 = r_dists.shape
        if self.nogc and C1 - 1 != self.num_predicates:
            raise ValueError("add_boxes: rel_dists has %d predicates, the evaluator %d"
                             % (C1 - 1, self.num_predicates))
        rels, lab, G, nobj = self._tables(gt_rels, gt_labels)
        idx = self._index(index)
        if G == 0:
            self._skipped.add(idx)
            return
        boxes = np.ascontiguousarray(np.asarray(gt_boxes, dtype=np.float32).reshape(nobj, 4))
        gtrip, gs, go, gpred, glab, ar, ks, gbox = self._upload(
            rels, lab, R, dev, extra=boxes.reshape(-1).view(np.int32))
        gbox = gbox.view(torch.float32).view(nobj, 4)       # (the bits of the float32 boxes)
        ptrip = torch.empty(R, 3, device=dev, dtype=torch.int32)
        score = torch.empty(R, device=dev, dtype=torch.float32)
        hip.pred_triplets(labels, r_dists, ptrip, score, R, C1)
        m = torch.empty(2, R, G, device=dev, dtype=torch.uint8)
        for ph in (0, 1):
            hip.triplet_match_boxes(ptrip, gtrip, R, G, det, det.stride(0), gbox, 4, ar[:R],
                                    ar[R:2 * R], gs, go, self.iou_thr, bool(ph), False, m[ph])
        rec = self._record(m[0], m[1], R, G, gpred, ks, dev)
        if self.nogc:
            K, nk = NOGC_TOP, len(self.ks)
            i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
            trip, srow, orow, count = i32(len(self.nogc), K, 3), i32(len(self.nogc), K), \
                i32(len(self.nogc), K), i32(len(self.nogc))
            nscore = torch.empty(len(self.nogc), K, device=dev, dtype=torch.float32)
            spare = i32(self.num_rel)             # (pn_eval_record writes the counts again)
            rd = r_dists.contiguous()
            for j, t in enumerate(self.nogc):
                P = min(K, R * t)                 # = count[j], known without reading it
                hip.nogc_triplets(det, det.stride(0), labels, rd, ar[:R], ar[R:2 * R], R, C1, t,
                                  K, trip[j], srow[j], orow[j], nscore[j], count[j:j + 1])
                mt = torch.empty(2, P, G, device=dev, dtype=torch.uint8)
                for ph in (0, 1):
                    hip.triplet_match_boxes(trip[j], gtrip, P, G, det, det.stride(0), gbox, 4,
                                            srow[j], orow[j], gs, go, self.iou_thr, bool(ph),
                                            False, mt[ph])
                o = self._nhits + self.num_rel + j * self._nhits
                hip.eval_record(mt[0], mt[1], P, G, gpred, ks, nk, self.num_rel,
                                rec[o:o + self._nhits], spare)
        valid = best = None
        if iou:
            valid = torch.empty(2 * nobj, device=dev, dtype=torch.uint8)
            best = torch.empty(2 * nobj, device=dev, dtype=torch.float64)
            hip.eval_iou_best_boxes(det, det.stride(0), labels, R, gbox, 4, glab, nobj, valid,
                                    best)
        self._log(idx, G, rec, valid, best, iou_rows=nobj)

    def add_host(self, index, image_eval, gt_rels, iou=None):
        """The same record computed in numpy from what `TripletEvaluator.__call__` /
        `evaluate_boxes` returned (`iou`: optionally its `iou_stats`): the restatement the
        kernels are tested against, and the entry of loops that run on the host."""
        rels = np.asarray(gt_rels).reshape(-1, 3)
        idx = self._index(index)
        if rels.shape[0] == 0:
            self._skipped.add(idx)
            return
        if rels[:, 2].min() < 1 or rels[:, 2].max() >= self.num_rel:
            raise ValueError("gt_rels: predicate ids must lie in [1, %d)" % self.num_rel)
        parts = host_record(image_eval, rels, self.num_rel, self.ks, nogc=self.nogc)
        if iou is None and "sub_iou" in image_eval:
            iou = (image_eval["sub_iou"], image_eval["obj_iou"])
        sub, obj = (np.zeros(0), np.zeros(0)) if iou is None else iou
        self._host[idx] = (int(rels.shape[0]), np.concatenate([p.reshape(-1) for p in parts]),
                           np.asarray(sub, np.float64).reshape(-1),
                           np.asarray(obj, np.float64).reshape(-1))

    # ---- the one place that waits for the GPU ----
    def _flush(self):
        if not self._dev:
            return
        dev = self._dev[0][2].device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            for _, _, rec, valid, best, ev, _ in self._dev:
                # add() may have run on other streams (the pipeline's chain streams): order
                # this stream behind each of them, and tell the allocator who reads the blocks
                cur.wait_event(ev)
                for t in (rec, valid, best):
                    if t is not None:
                        t.record_stream(cur)
            recs = torch.stack([d[2] for d in self._dev]).cpu().numpy()
            with_iou = [d for d in self._dev if d[3] is not None]
            if with_iou:
                valid = torch.cat([d[3] for d in with_iou]).cpu().numpy().astype(bool)
                best = torch.cat([d[4] for d in with_iou]).cpu().numpy()
        o = 0
        for i, (idx, G, _, v, _, _, rows) in enumerate(self._dev):
            sub = obj = np.zeros(0)
            if v is not None:                 # rows per side: G (masks) or n_obj (boxes)
                sub = best[o:o + rows][valid[o:o + rows]]
                obj = best[o + rows:o + 2 * rows][valid[o + rows:o + 2 * rows]]
                o += 2 * rows
            self._host[idx] = (G, recs[i], sub, obj)
        self._dev = []

    def records(self):
        """{index: dict(G, hits [2][nk][num_rel], counts [num_rel], sub_iou, obj_iou)} of the
        images added so far (waits for the GPU); with `nogc` also nogc_hits
        {threshold: [2][nk][num_rel]}."""
        self._flush()
        n, nr, shape = self._nhits, self.num_rel, (2, len(self.ks), self.num_rel)
        out = {}
        for idx, (G, ints, sub, obj) in self._host.items():
            out[idx] = dict(G=G, hits=ints[:n].reshape(shape), counts=ints[n:n + nr],
                            sub_iou=sub, obj_iou=obj)
            if self.nogc:
                out[idx]["nogc_hits"] = {
                    t: ints[n + nr + j * n:n + nr + (j + 1) * n].reshape(shape)
                    for j, t in enumerate(self.nogc)}
        return out

    def state(self):
        """Everything added so far as ONE float64 array (int32 values are exact in it):
        [magic, images, skipped, nk, num_rel | per image: index, G, n_sub, n_obj, record,
        sub IoUs, obj IoUs | skipped indices].  The only place the class waits for the GPU;
        three device-to-host copies however many images there are.  With `nogc` the magic word
        is another one, the header goes on with [number of thresholds, thresholds...], and the
        record is the longer one (`host_record(..., nogc=...)`)."""
        self._flush()
        magic, config = self._config()
        parts = [np.array([magic, len(self._host), len(self._skipped)] + config, np.float64)]
        for idx in sorted(self._host):
            G, ints, sub, obj = self._host[idx]
            parts += [np.array([idx, G, sub.shape[0], obj.shape[0]], np.float64),
                      ints.astype(np.float64), sub, obj]
        parts.append(np.array(sorted(self._skipped), np.float64))
        return np.concatenate(parts)

    def merge(self, states):
        """Replace this evaluator's contents by the union of `states` (the `state()` blobs of
        all ranks, its own among them).  An image present in two blobs is an error."""
        self._flush()
        host, skipped = {}, set()
        n = self._nints
        magic, config = self._config()
        head = 3 + len(config)
        for blob in states:
            blob = np.asarray(blob, np.float64)
            if blob.shape[0] < head or int(blob[0]) != magic or \
                    [int(v) for v in blob[3:head]] != config:
                raise ValueError("StreamingEvaluator.merge: not a state of this configuration")
            o = head
            for _ in range(int(blob[1])):
                idx, G, ns, no = (int(v) for v in blob[o:o + 4])
                o += 4
                if idx in host or idx in skipped:
                    raise ValueError("StreamingEvaluator.merge: image %d occurs twice" % idx)
                host[idx] = (G, blob[o:o + n].astype(np.int32), blob[o + n:o + n + ns].copy(),
                             blob[o + n + ns:o + n + ns + no].copy())
                o += n + ns + no
            for v in blob[o:o + int(blob[2])]:
                if int(v) in host or int(v) in skipped:
                    raise ValueError("StreamingEvaluator.merge: image %d occurs twice" % int(v))
                skipped.add(int(v))
        self._host, self._skipped = host, skipped
        self._seen = set(host) | skipped

    def summary(self):
        """What `SceneGraphMetrics.summary()` returns after the same images were added to it
        in dataset order: its lists are rebuilt from the records with the reference's float
        expressions (`hits / float(G)`, `float(hit / count)`), its own code does the rest."""
        self._flush()
        m = SceneGraphMetrics(self.num_predicates, self.ks, nogc=self.nogc or None)
        nk, nr, nh = len(self.ks), self.num_rel, self._nhits

        def rebuild(hits, counts, G, recalls, collect):
            for mi, mode in enumerate(("sgdet", "phrdet")):
                for j, k in enumerate(self.ks):
                    recalls[mode][k].append(int(hits[mi, j, 0]) / float(G))
                    for n in range(nr):
                        if counts[n] > 0:
                            collect[mode][k][n].append(float(int(hits[mi, j, n]) / int(counts[n])))

        for idx in sorted(self._host):
            G, ints, sub, obj = self._host[idx]
            counts = ints[nh:nh + nr]
            m.images += 1
            rebuild(ints[:nh].reshape(2, nk, nr), counts, G, m.recalls, m.collect)
            for j, t in enumerate(self.nogc):
                o = nh + nr + j * nh
                rebuild(ints[o:o + nh].reshape(2, nk, nr), counts, G, m.nogc_recalls[t],
                        m.nogc_collect[t])
            m.sub_iou.extend(sub)
            m.obj_iou.extend(obj)
        m.skipped = len(self._skipped)
        return m.summary()


# ---- panoptic quality ----------------------------------------------------------------------
PQ_BAD_VALUE, PQ_BAD_SEGMENT, PQ_TWO_CATEGORIES, PQ_BAD_GT_CATEGORY = 1, 2, 4, 8
_PQ_STATUS = ((PQ_BAD_VALUE, "a value below 0 or with a class above num_classes"),
              (PQ_BAD_SEGMENT, "a segment index of 256 or more"),
              (PQ_TWO_CATEGORIES, "two classes under one segment index"),
              (PQ_BAD_GT_CATEGORY, "a ground-truth category outside [0, num_classes)"))


def rgb2id(rgb):
    """The panoptic PNG's ids: R + 256 G + 65536 B of an (H, W, 3) uint8 array, int64."""
    rgb = np.asarray(rgb).astype(np.int64)
    return rgb[..., 0] + 256 * rgb[..., 1] + 65536 * rgb[..., 2]


def host_confusion(pred, gt_ids, seg, num_classes, instance_offset):
    """`pn_pq_confusion` in numpy: (N [(G + 1)][257] int32, col_cat [256] int32, status).
    seg: (G, 3) (id, category, iscrowd) sorted by id.  Row 0 / column 256 are void."""
    v = np.asarray(pred).astype(np.int64).reshape(-1)
    gid = np.asarray(gt_ids).astype(np.int64).reshape(-1)
    G = seg.shape[0]
    neg = v < 0
    s, c = np.where(neg, 0, v) // instance_offset, np.where(neg, 0, v) % instance_offset
    bad_c, bad_s = neg | (c > num_classes), ~neg & (s >= 256)
    status = (PQ_BAD_VALUE if bad_c.any() else 0) | (PQ_BAD_SEGMENT if bad_s.any() else 0)
    ok = ~(bad_c | bad_s)
    seg_px = ok & (c < num_classes)
    col_cat = np.full(256, -1, np.int32)
    np.maximum.at(col_cat, s[seg_px], c[seg_px].astype(np.int32))
    if (col_cat[s[seg_px]] != c[seg_px]).any():
        status |= PQ_TWO_CATEGORIES
    col = np.where(seg_px, s, 256)
    pos = np.searchsorted(seg[:, 0], gid)
    hit = (gid != 0) & (pos < G)
    hit[hit] = seg[pos[hit], 0] == gid[hit]
    row = np.where(hit, pos + 1, 0)
    N = np.bincount((row * 257 + col)[ok], minlength=(G + 1) * 257)
    return N.reshape(G + 1, 257).astype(np.int32), col_cat, status


def host_pq_record(N, col_cat, seg, num_classes):
    """`pn_pq_record` in numpy: (rec [num_classes][3] int32 = tp, fp, fn; iou [num_classes]
    float64; match [G + 1])."""
    N = N.astype(np.int64)
    G = seg.shape[0]
    area_g, area_p = N.sum(1), N.sum(0)
    cat, crowd = seg[:, 1], seg[:, 2] != 0
    union = area_p[None, :256] + area_g[1:, None] - N[1:, :256] - N[0:1, :256]
    same = (cat[:, None] == col_cat[None, :].astype(np.int64)) & ~crowd[:, None]
    hit = same & (N[1:, :256] > 0) & (2 * N[1:, :256] > union)
    if G and (hit.sum(0).max() > 1 or hit.sum(1).max() > 1):
        raise AssertionError("two matches for one segment: iou > 0.5 cannot hold twice")
    rec = np.zeros((num_classes, 3), np.int32)
    iou = np.zeros(num_classes, np.float64)
    match = np.full(G + 1, -1, np.int32)
    for g in range(G):                         # ascending ground-truth id
        if crowd[g]:
            continue
        p = np.nonzero(hit[g])[0]
        if p.shape[0]:
            match[g + 1] = p[0]
            rec[cat[g], 0] += 1
            iou[cat[g]] += np.float64(N[g + 1, p[0]]) / np.float64(union[g, p[0]])
        else:
            rec[cat[g], 2] += 1
    unmatched = (col_cat >= 0) & (area_p[:256] > 0) & ~hit.any(0)
    for p in np.nonzero(unmatched)[0]:
        absorbed = N[0, p] + N[1:, p][crowd & (cat == col_cat[p])].sum()
        if not 2 * absorbed > area_p[p]:
            rec[col_cat[p], 1] += 1
    return rec, iou, match


class PanopticQuality:
    """PQ / SQ / RQ of the panoptic maps `get_bboxes` returns as field 4 (`Result.pan_results`):
    the metric of the reference's `--eval PQ` (pairnet/datasets/psg.py:309-335 -> mmdet's panoptic
    evaluation), restated from memory (INTEGRATION.md 3a-2 is the specification), for a loop that
    must not wait for the GPU.  `add()` enqueues one pass over the pixels (`pn_pq_confusion`: the
    ground-truth x predicted segment overlap table) and the matching (`pn_pq_record`) on the
    current stream and leaves the image's record -- (tp, fp, fn) per category as int32, the IoU
    sums as float64 -- and a status word on the device; nothing is read back before `state()` /
    `summary()`.

        pq = PanopticQuality()                       # PSG: 133 classes, 80 of them things
        for each image i:  pq.add(result[4], gt_pan_rgb, gt_segments, index=i)
        pq.summary()   ->  {"PQ": .., "SQ": .., "RQ": .., "PQ_th": .., ..., "PQ_st": .., ...,
                            "n": {"all": .., "things": .., "stuff": ..}, "images": n,
                            "classwise": {category: (pq, sq, rq)}}     (percentages)

    Several ranks: `pq.merge(all ranks' pq.state())` on rank 0, then `pq.summary()`; records are
    summed in ascending image index, so the result equals a single-rank run bit for bit.
    `keep_confusion`: keep every image's table N for `records()` (tests; ~1 KB per ground-truth
    segment and image of device memory until the flush)."""

    _MAGIC = 0x5051

    def __init__(self, num_classes=133, num_things=80, instance_offset=1000,
                 keep_confusion=False):
        self.num_classes, self.num_things = int(num_classes), int(num_things)
        self.instance_offset = int(instance_offset)   # head.INSTANCE_OFFSET
        if not 1 <= self.num_classes <= 999 or not 0 <= self.num_things <= self.num_classes \
                or self.instance_offset <= self.num_classes:
            raise ValueError("PanopticQuality: 1 <= num_classes <= 999 < instance_offset")
        self.keep_confusion = bool(keep_confusion)
        self._host = {}       # index -> (status, ints [3 num_classes] int32, iou f64, N or None)
        self._dev = []        # (index, ints + status, iou, N or None, event): not read back yet
        self._seen = set()
        self._calls = 0

    def _segments(self, gt_segments):
        """(G, 3) int64 (id, category, iscrowd) sorted by id, from an array or from the
        `segments_info` dicts; checked on the host."""
        if torch.is_tensor(gt_segments):
            if gt_segments.is_cuda:
                raise ValueError("gt_segments is host data (only the maps live on the device)")
            gt_segments = gt_segments.numpy()
        if len(gt_segments) and isinstance(gt_segments[0], dict):
            gt_segments = [(s["id"], s["category_id"], s.get("iscrowd", 0)) for s in gt_segments]
        seg = np.asarray(gt_segments, dtype=np.int64).reshape(-1, 3)
        seg = seg[np.argsort(seg[:, 0], kind="stable")]
        if seg.shape[0] > 255:
            raise ValueError("PanopticQuality: at most 255 ground-truth segments per image")
        if seg.shape[0] and (seg[0, 0] < 1 or seg[-1, 0] >= 1 << 24 or
                             (np.diff(seg[:, 0]) == 0).any()):
            raise ValueError("gt_segments: ids must be distinct and lie in [1, 2^24)")
        if seg.shape[0] and (seg[:, 1].min() < 0 or seg[:, 1].max() >= self.num_classes):
            raise ValueError("gt_segments: categories must lie in [0, %d)" % self.num_classes)
        return seg

    def _index(self, index):
        idx = self._calls if index is None else int(index)
        self._calls += 1
        if idx in self._seen:
            raise ValueError("PanopticQuality: image %d was added before" % idx)
        self._seen.add(idx)
        return idx

    @torch.no_grad()
    @hip.on_device
    def add(self, pan_seg, gt_pan_rgb, gt_segments, index=None, flags=0):
        """pan_seg: the device map [H, W] int64 (`result[4]`, or the 8-tuple itself);
        gt_pan_rgb: the panoptic PNG (H, W, 3) uint8, on the device as
        `dataset.panoptic_ground_truth` leaves it (a host array goes up pinned, non-blocking);
        gt_segments: host data, (G, 3) (id, category, iscrowd) or the `segments_info` dicts.
        Everything is enqueued on the current stream; nothing is read back."""
        if isinstance(pan_seg, (tuple, list)):
            pan_seg = pan_seg[4]
        if not torch.is_tensor(pan_seg) or not pan_seg.is_cuda or pan_seg.dim() != 2 or \
                pan_seg.dtype != torch.int64:
            raise ValueError("pan_seg: a device tensor [H, W] int64")
        dev = pan_seg.device
        gt = gt_pan_rgb if torch.is_tensor(gt_pan_rgb) else \
            torch.from_numpy(np.ascontiguousarray(gt_pan_rgb))
        if gt.dtype != torch.uint8 or gt.dim() != 3 or gt.shape[2] != 3:
            raise ValueError("gt_pan_rgb: the panoptic PNG as (H, W, 3) uint8")
        if tuple(gt.shape[:2]) != tuple(pan_seg.shape):
            raise ValueError("PanopticQuality: prediction %s and ground truth %s differ in size"
                             % (tuple(pan_seg.shape), tuple(gt.shape[:2])))
        if pan_seg.numel() == 0 or pan_seg.numel() >= 1 << 31:
            raise ValueError("PanopticQuality: 0 < H * W < 2^31")
        seg = self._segments(gt_segments)
        idx = self._index(index)
        G, nc = seg.shape[0], self.num_classes
        if not gt.is_cuda:
            gt = gt.contiguous().pin_memory().to(dev, non_blocking=True)
        gt = gt.contiguous()
        pred = pan_seg.contiguous()
        if pred.data_ptr() % 16:
            pred = pred.clone()
        if gt.data_ptr() % 4:
            gt = gt.clone()
        n = max(G, 1)                              # [ids | categories | iscrowd], one copy
        host = np.zeros((3, n), np.int32)
        host[:, :G] = seg.T
        buf = torch.empty((3, n), dtype=torch.int32, pin_memory=True)
        buf.copy_(torch.from_numpy(host))
        tab = buf.to(dev, non_blocking=True)
        i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
        N, col_cat = i32((G + 1) * hip.PQ_COLS), i32(256)
        ints = i32(3 * nc + 1)                     # the record, then the status word
        iou = torch.empty(nc, device=dev, dtype=torch.float64)
        hip.pq_confusion(pred, gt, tab[0], G, nc, self.instance_offset, N, col_cat,
                         ints[3 * nc:], flags=flags)
        hip.pq_record(N, col_cat, tab[1], tab[2], G, nc, i32(G + 1), i32(hip.PQ_COLS),
                      i32(G + 1), ints[:3 * nc], iou, ints[3 * nc:])
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self._dev.append((idx, ints, iou, N if self.keep_confusion else None, ev))

    def add_host(self, index, pred, gt_ids, gt_segments):
        """The same record computed in numpy from host maps: pred [H, W] integer, gt_ids [H, W]
        the ground-truth id map (`rgb2id` of the PNG).  The restatement the kernels are tested
        against, and the entry of loops that run on the host."""
        pred = pred.cpu().numpy() if torch.is_tensor(pred) else np.asarray(pred)
        gt_ids = gt_ids.cpu().numpy() if torch.is_tensor(gt_ids) else np.asarray(gt_ids)
        if pred.ndim != 2 or pred.shape != gt_ids.shape:
            raise ValueError("PanopticQuality: prediction %s and ground truth %s differ in size"
                             % (pred.shape, gt_ids.shape))
        seg = self._segments(gt_segments)
        idx = self._index(index)
        N, col_cat, status = host_confusion(pred, gt_ids, seg, self.num_classes,
                                            self.instance_offset)
        rec, iou, _ = host_pq_record(N, col_cat, seg, self.num_classes)
        self._host[idx] = (int(status), rec.reshape(-1), iou, N if self.keep_confusion else None)

    # ---- the one place that waits for the GPU ----
    def _flush(self):
        if not self._dev:
            return
        dev = self._dev[0][1].device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            for _, ints, iou, N, ev in self._dev:
                # add() may have run on other streams (the pipeline's chain streams): order
                # this stream behind each of them, and tell the allocator who reads the blocks
                cur.wait_event(ev)
                for t in (ints, iou, N):
                    if t is not None:
                        t.record_stream(cur)
            ints = torch.stack([d[1] for d in self._dev]).cpu().numpy()
            ious = torch.stack([d[2] for d in self._dev]).cpu().numpy()
            tables = [None if d[3] is None else d[3].cpu().numpy().reshape(-1, hip.PQ_COLS)
                      for d in self._dev]
        for i, d in enumerate(self._dev):
            self._host[d[0]] = (int(ints[i, -1]), ints[i, :-1].copy(), ious[i].copy(), tables[i])
        self._dev = []

    def records(self):
        """{index: dict(status, rec [num_classes][3] int32 (tp, fp, fn), iou [num_classes]
        float64, N [(G + 1)][257] or None)} of the images added so far (waits for the GPU)."""
        self._flush()
        return {idx: dict(status=st, rec=ints.reshape(self.num_classes, 3), iou=iou, N=N)
                for idx, (st, ints, iou, N) in self._host.items()}

    def _header(self):
        return [self._MAGIC, self.num_classes, self.num_things, self.instance_offset]

    def state(self):
        """Everything added so far as ONE float64 array (int32 values are exact in it):
        [magic, num_classes, num_things, instance_offset, images | per image in ascending
        index: index, status, record, IoU sums]."""
        self._flush()
        parts = [np.array(self._header() + [len(self._host)], np.float64)]
        for idx in sorted(self._host):
            st, ints, iou, _ = self._host[idx]
            parts += [np.array([idx, st], np.float64), ints.astype(np.float64), iou]
        return np.concatenate(parts)

    def merge(self, states):
        """Replace this object's contents by the union of `states` (the `state()` blobs of all
        ranks, its own among them).  An image present in two blobs is an error."""
        self._flush()
        host, nc = {}, self.num_classes
        for blob in states:
            blob = np.asarray(blob, np.float64)
            if blob.ndim != 1 or blob.shape[0] < 5 or \
                    [int(v) for v in blob[:4]] != self._header() or \
                    blob.shape[0] != 5 + int(blob[4]) * (2 + 4 * nc):
                raise ValueError("PanopticQuality.merge: not a state of this configuration")
            o = 5
            for _ in range(int(blob[4])):
                idx, st = int(blob[o]), int(blob[o + 1])
                if idx in host:
                    raise ValueError("PanopticQuality.merge: image %d occurs twice" % idx)
                host[idx] = (st, blob[o + 2:o + 2 + 3 * nc].astype(np.int32),
                             blob[o + 2 + 3 * nc:o + 2 + 4 * nc].copy(), None)
                o += 2 + 4 * nc
        self._host = host
        self._seen = set(host)

    def summary(self):
        """Per category tp / fp / fn summed as integers and the IoU sums added as float64 in
        ascending image index; pq = iou / (tp + fp / 2 + fn / 2), sq = iou / tp, rq = tp /
        (tp + fp / 2 + fn / 2); averaged over the categories with tp + fp + fn > 0 (in ascending
        category), times 100.  An image whose status word is set raises here."""
        self._flush()
        nc = self.num_classes
        for idx in sorted(self._host):
            st = self._host[idx][0]
            if st:
                raise ValueError("PanopticQuality: the panoptic map of image %d has %s (status %d)"
                                 % (idx, "; ".join(w for b, w in _PQ_STATUS if st & b), st))
        cnt = np.zeros((nc, 3), np.int64)
        iou = np.zeros(nc, np.float64)
        for idx in sorted(self._host):
            _, ints, io, _ = self._host[idx]
            cnt += ints.reshape(nc, 3)
            iou += io
        classwise = {}
        for c in range(nc):
            tp, fp, fn = (int(v) for v in cnt[c])
            if tp + fp + fn == 0:
                continue
            den = tp + 0.5 * fp + 0.5 * fn
            classwise[c] = (float(iou[c]) / den, float(iou[c]) / tp if tp else 0.0, tp / den)
        out = dict(images=len(self._host), classwise=classwise, n={})
        for name, suffix, keep in (("all", "", lambda c: True),
                                   ("things", "_th", lambda c: c < self.num_things),
                                   ("stuff", "_st", lambda c: c >= self.num_things)):
            rows = [classwise[c] for c in sorted(classwise) if keep(c)]
            out["n"][name] = len(rows)
            for j, key in enumerate(("PQ", "SQ", "RQ")):
                out[key + suffix] = 100.0 * (sum(r[j] for r in rows) / len(rows)) if rows else 0.0
        return out
