"""The loss of `PSGTrHead2` on device outputs: the seven terms `s_loss_cls`, `o_loss_cls`,
`r_loss_cls`, `s_loss_mask`, `o_loss_mask`, `s_loss_dice`, `o_loss_dice` of the reference's
`PSGTrHead2.loss` (pairnet/models/relation_heads/psgtr_head2.py:447-1018 with `MaskHTriMatcher`,
approaches/matcher.py:10-102) under configs/psgtr/psgtr_r50_psg_plus.py:118-177.

`PSGTrHead2Loss.loss(...)` takes the two dicts `PSGTrHead2.forward` returns (`sub` / `obj`
[1, B, Q, C + 1], `rel` [1, B, Q, Cr + 1]; `sub_seg` / `obj_seg` [1, B, Q, h, w]: the leading 1 is
the reference's `torch.stack(...)[-1:]`, :433-441, so there is one "layer" and seven unprefixed keys)
and the per-image ground truth in the reference's argument order, and returns the seven terms as
0-dim device tensors: the VALUES and, with `grads={}`, the gradient of their SUM with respect to the
five logit blocks.  Carrying those gradients on into the embeddings and the decoder is not built
(DESIGN 7b).

Per call: `pn_tri_match_cost_f32` (csrc/tri_loss.hip) fills every image's [Q, R_b] cost block --
one draw of `num_points` points per image shared by subject and object, predictions and ground truth
(:909); the mask and dice terms once per (side, query, OBJECT), gathered per relation through
`gt_rels`; five launches -- ONE `pn_lsa_f32` launch solves the B assignments, `pn_tri_targets` writes the three
label vectors and the matched rows.  The loss side reuses csrc/seg_loss.hip unchanged, each mask side
as one "layer" of its own call (the two mask stacks of the head are separate allocations; nothing is
copied): `pn_ce_avg_f32` three times, `pn_uncertain_points_f32`, `pn_point_sample_rows_f32`,
`pn_mask_point_loss_f32` and `pn_point_scatter_grad_f32` per side.  The number of launches does not
depend on B, on the relations or on the objects.

Reference behaviour kept on purpose:
  * unmatched queries get relation label `num_relations`, the LAST index (:981-984), while
    `bg_cls_weight` sits at index 0 of the relation class weights (:134-137): they are pushed to the
    last predicate at weight `class_weight`, not to a background at 0.02;
  * `s_loss_cls`'s avg_factor is taken from the OBJECT class weights (:680-688); configs whose
    subject and object `class_weight` differ are refused here.
An image without a ground-truth relation fails in the reference (`torch.cat([])`, :919) and raises
ValueError here, so the reference's zero-match branch (:721-725) cannot be reached and is not built;
`use_mask=False` runs into an undefined name there (:520) and is refused by the head.

The draws are counter-based (`pn_uniform_f32` at the five `hip.TRI_SITE_*`); `points=` injects the
reference's `torch.rand` draws instead.  Nothing crosses PCIe except the ground truth going up
(pinned, non-blocking) and nothing is waited for: a cost matrix scipy would raise on sets
`self.assign_status` (a device word, bits in include/pairnet_hip.h) and leaves that image's labels at
their fills and its rows out.  A side above `hip.LSA_MAX_SIDE` (known from shapes) takes scipy on the
host.  `num_total_masks` is this rank's own count; a data-parallel caller passes its all-reduced mean
(the reference's `reduce_mean`, :716-718).  No collective here.
"""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import hip
from .config import ConfigDict, psgtr2_train_cfg
from .losses import _to_dev
from .seg_losses import Mask2FormerLoss

_BUILT = "configs/psgtr/psgtr_r50_psg_plus.py:118-177"
_COSTS = (("s_cls_cost", "ClassificationCost"), ("s_mask_cost", "CrossEntropyLossCost"),
          ("s_dice_cost", "DiceCost"), ("o_cls_cost", "ClassificationCost"),
          ("o_mask_cost", "CrossEntropyLossCost"), ("o_dice_cost", "DiceCost"),
          ("r_cls_cost", "ClassificationCost"))
_POINT_KEYS = ("assign", "sub_candidates", "sub_tail", "obj_candidates", "obj_tail", "sub_loss",
               "obj_loss")


class PSGTrHead2Loss:
    def __init__(self, num_classes, num_relations, num_queries, bg_cls_weight=0.02, train_cfg=None,
                 sub_loss_cls=None, sub_loss_mask=None, sub_loss_dice=None, obj_loss_cls=None,
                 obj_loss_mask=None, obj_loss_dice=None, rel_loss_cls=None):
        t = ConfigDict(train_cfg or psgtr2_train_cfg())
        ce = lambda w: dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=w,
                            class_weight=1.0)
        mask = dict(type="CrossEntropyLoss", use_sigmoid=True, reduction="mean", loss_weight=5.0)
        dice = dict(type="DiceLoss", use_sigmoid=True, activate=True, reduction="mean",
                    naive_dice=True, eps=1.0, loss_weight=5.0)
        sc, oc, rc = dict(sub_loss_cls or ce(1.0)), dict(obj_loss_cls or ce(1.0)), \
            dict(rel_loss_cls or ce(2.0))
        sm, om = dict(sub_loss_mask or mask), dict(obj_loss_mask or mask)
        sd, od = dict(sub_loss_dice or dice), dict(obj_loss_dice or dice)
        ma = t.get("assigner")
        if ma is None:
            raise NotImplementedError("train_cfg without an assigner (built: MaskHTriMatcher, %s)"
                                      % _BUILT)
        costs = [dict(ma.get(k) or {}) for k, _ in _COSTS]
        want = [(ma.get("type"), "MaskHTriMatcher")] + \
            [(c.get("type"), exp) for c, (_, exp) in zip(costs, _COSTS)] + \
            [(t.get("sampler", dict(type="MaskPseudoSampler"))["type"], "MaskPseudoSampler")] + \
            [(c.get("type"), "CrossEntropyLoss") for c in (sc, oc, rc, sm, om)] + \
            [(c.get("type"), "DiceLoss") for c in (sd, od)]
        for got, exp in want:
            if got != exp:
                raise NotImplementedError("%s (built: %s, %s)" % (got, exp, _BUILT))
        if any(not c.get("use_sigmoid", True) for c in (costs[1], costs[4])) \
                or any(not c.get("pred_act", False) or not c.get("naive_dice", True)
                       for c in (costs[2], costs[5])) \
                or any(c.get("use_sigmoid", False) or c.get("use_mask", False) for c in (sc, oc, rc)) \
                or any(not c.get("use_sigmoid", False) for c in (sm, om)) \
                or any(not c.get("use_sigmoid", True) or not c.get("activate", True)
                       or not c.get("naive_dice", False) for c in (sd, od)) \
                or any(c.get("reduction", "mean") != "mean" for c in (sc, oc, rc, sm, om, sd, od)) \
                or any(c.get("class_weight") is not None for c in (sm, om, sd, od)) \
                or any(c.get("ignore_index") is not None or c.get("avg_non_ignore", False)
                       for c in (sc, oc, rc, sm, om)):
            raise NotImplementedError("cost / loss options outside what is built (%s)" % _BUILT)
        for name, c in (("sub_loss_cls", sc), ("obj_loss_cls", oc), ("rel_loss_cls", rc)):
            # (the reference asserts a float and builds the weight vector itself, psgtr_head2.py:103-138)
            if not isinstance(c.get("class_weight"), float):
                raise NotImplementedError("%s.class_weight must be a float (built: %s), got %r"
                                          % (name, _BUILT, c.get("class_weight")))
        if not isinstance(bg_cls_weight, float):
            raise NotImplementedError("bg_cls_weight must be a float, got %r" % (bg_cls_weight,))
        if sc["class_weight"] != oc["class_weight"]:
            # (s_loss_cls's avg_factor reads the OBJECT class weights, psgtr_head2.py:680-688: with
            # equal weights that is the usual normalisation, and only that is built)
            raise NotImplementedError("sub_loss_cls.class_weight != obj_loss_cls.class_weight "
                                      "(psgtr_head2.py:680-688 normalises s_loss_cls by the object "
                                      "weights; built: equal weights, %s)" % _BUILT)
        self.num_classes, self.num_relations = int(num_classes), int(num_relations)
        self.Q = int(num_queries)
        self.num_points = int(t.get("num_points", 12544))
        self.oversample_ratio = float(t.get("oversample_ratio", 3.0))
        self.importance_sample_ratio = float(t.get("importance_sample_ratio", 0.75))
        if self.oversample_ratio < 1 or not 0 <= self.importance_sample_ratio <= 1:
            raise ValueError("oversample_ratio >= 1 and 0 <= importance_sample_ratio <= 1 "
                             "(point_sample.py:57-58)")
        # s_cls, s_mask, s_dice, o_cls, o_mask, o_dice, r_cls weights, then the two dice eps
        self.cost_weights = [float(c.get("weight", 1.0)) for c in costs] + \
            [float(costs[2].get("eps", 1e-3)), float(costs[5].get("eps", 1e-3))]
        C, Cr = self.num_classes, self.num_relations
        self.bg_cls_weight = bg_cls_weight
        # (:110-137) background LAST for subjects / objects, FIRST for relations
        self.sub_class_weight = [sc["class_weight"]] * C + [bg_cls_weight]
        self.obj_class_weight = [oc["class_weight"]] * C + [bg_cls_weight]
        self.rel_class_weight = [bg_cls_weight] + [rc["class_weight"]] * Cr
        self.w_cls = tuple(float(c.get("loss_weight", 1.0)) for c in (sc, oc, rc))
        self.w_mask = tuple(float(c.get("loss_weight", 1.0)) for c in (sm, om))
        self.w_dice = tuple(float(c.get("loss_weight", 1.0)) for c in (sd, od))
        self.dice_eps = tuple(float(c.get("eps", 1e-3)) for c in (sd, od))
        self._cw = None
        self.assign_status = None      # device int32 [1] of the last call
        self.last_on_device = False    # whether the last call solved its assignments on the device
        self.last = None               # the last call's targets (device tensors)

    _ground_truth = Mask2FormerLoss._ground_truth       # (labels, one uint8 mask stack, G_b)

    def _relations(self, gt_rels_list, G):
        rels = []
        for b, gr in enumerate(gt_rels_list):
            gr = torch.as_tensor(gr)
            if gr.numel() == 0:
                # (the reference fails at torch.cat([]), psgtr_head2.py:919)
                raise ValueError("image %d has no ground-truth relation" % b)
            if gr.dim() != 2 or gr.shape[1] != 3:
                raise ValueError("gt_rels: [R, 3], got %s" % (tuple(gr.shape),))
            gr = gr.to(torch.int64)
            if not gr.is_cuda:      # (a device tensor is range-checked on the device: status bit 4)
                if int(gr[:, :2].min()) < 0 or int(gr[:, :2].max()) >= G[b]:
                    raise ValueError("image %d: gt_rels objects outside [0, %d)" % (b, G[b]))
                if int(gr[:, 2].min()) < 1 or int(gr[:, 2].max()) > self.num_relations:
                    raise ValueError("image %d: gt_rels predicates outside [1, %d]"
                                     % (b, self.num_relations))
            rels.append(gr)
        return rels

    @torch.no_grad()
    @hip.on_device
    def loss(self, all_cls_scores, all_mask_preds, gt_rels_list, gt_bboxes_list, gt_labels_list,
             gt_masks_list, img_metas, gt_bboxes_ignore=None, grads=None, points=None, seed=0, step=0,
             num_total_masks=None, rank=0, debug=False):
        """The reference's argument order (psgtr_head2.py:447-457); `gt_bboxes_list` is not read.
        `points`: the reference's draws, to reproduce one of its runs -- dict(assign=[B] of [Np, 2],
        sub_candidates / obj_candidates [M, S, 2], sub_tail / obj_tail [M, Np - k, 2]) or, instead of
        a side's candidates and tail, sub_loss / obj_loss [M, Np, 2] (final loss points, selection
        bypassed); every key is optional, a missing one is drawn here.  `grads`: a dict filled with
        "sub", "obj", "rel" (shaped like the inputs), "mask_rows" int64 [M] (row into B * Q, the same
        rows for both sides; -1 where the image's assignment failed) and "sub_mask" / "obj_mask"
        [M, h, w].  `self.last` keeps sub_labels / obj_labels / rel_labels [B * Q], matched [M, 4] =
        (image, query, subject object, object object; objects counted over the batch), rel_idx [M]
        (the matched relation's index in its image), mcount and `counts`, the host list
        min(Q, R_b); `debug=True` also keeps the cost blocks, the assignment, the points and the
        samples alive there."""
        if gt_bboxes_ignore is not None:
            raise AssertionError("Only supports for gt_bboxes_ignore setting to None.")
        cls = [all_cls_scores[k] for k in ("sub", "obj", "rel")]
        seg = [all_mask_preds[k] for k in ("sub_seg", "obj_seg")]
        C1, Cr1, Q = self.num_classes + 1, self.num_relations + 1, self.Q
        ok = all(torch.is_tensor(t) and t.dtype == torch.float32 for t in cls + seg) and \
            cls[0].dim() == 4 and cls[0].shape[0] == 1 and seg[0].dim() == 5
        if ok:
            B = int(cls[0].shape[1])
            h, w = int(seg[0].shape[3]), int(seg[0].shape[4])
            ok = tuple(cls[0].shape) == (1, B, Q, C1) and tuple(cls[1].shape) == (1, B, Q, C1) and \
                tuple(cls[2].shape) == (1, B, Q, Cr1) and \
                all(tuple(s.shape) == (1, B, Q, h, w) for s in seg)
        if not ok:
            raise ValueError("sub / obj [1, B, %d, %d], rel [1, B, %d, %d] and sub_seg / obj_seg "
                             "[1, B, %d, h, w] fp32 logits (what PSGTrHead2.forward returns), got %s"
                             % (Q, C1, Q, Cr1, Q, [tuple(t.shape) if torch.is_tensor(t)
                                                   else type(t).__name__ for t in cls + seg]))
        if B * Q > 4096:
            raise NotImplementedError("B * Q <= 4096 rows per call")
        points = dict(points or {})
        unknown = set(points) - set(_POINT_KEYS)
        if unknown:
            raise ValueError("points: unknown keys %s" % sorted(unknown))
        if len(gt_rels_list) != B or len(gt_labels_list) != B or len(gt_masks_list) != B:
            raise ValueError("ground truth for %d / %d / %d images, logits for %d"
                             % (len(gt_rels_list), len(gt_labels_list), len(gt_masks_list), B))
        G = [int(torch.as_tensor(l).numel()) for l in gt_labels_list]
        rels = self._relations(gt_rels_list, G)          # (raises before anything is launched)
        dev = cls[0].device
        labels_h, gt_all, G = self._ground_truth(gt_labels_list, gt_masks_list, B, h, w, dev)
        if min(G) == 0:
            raise ValueError("an image with relations has no ground-truth object")
        hg, wg = int(gt_all.shape[1]), int(gt_all.shape[2])
        f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
        sub, obj, rel = (t.contiguous().view(B, Q, -1) for t in cls)
        s_seg, o_seg = (t.contiguous().view(B, Q, h, w) for t in seg)

        # ---- sizes and the two tables, on the host from shapes alone; one upload ----
        R = [int(g.shape[0]) for g in rels]
        P_b = [min(Q, r) for r in R]
        M = sum(P_b)
        if M > 65535:
            raise NotImplementedError("at most 65535 matched masks per call")
        tab, lsa_tab = [], []
        c_off = r_off = g_off = o_off = 0
        for b in range(B):
            tab += [c_off, R[b], r_off, g_off, G[b], o_off, 0, 0]
            lsa_tab += [c_off, Q, R[b], o_off]
            c_off, r_off, g_off, o_off = c_off + Q * R[b], r_off + R[b], g_off + G[b], o_off + P_b[b]
        head = torch.tensor(tab + lsa_tab, dtype=torch.int64)
        nh = head.numel()
        if all(not t.is_cuda for t in rels + labels_h):
            buf = torch.empty(nh + 3 * r_off + g_off, dtype=torch.int64, pin_memory=True)
            torch.cat([head] + [t.reshape(-1) for t in rels] + labels_h, out=buf)
            up = buf.to(dev, non_blocking=True)
            tabs, gt_rels, gl = up[:nh], up[nh:nh + 3 * r_off].view(r_off, 3), up[nh + 3 * r_off:]
        else:
            tabs = _to_dev(head, dev)
            gt_rels = torch.cat([_to_dev(t, dev) for t in rels]).contiguous()
            gl = torch.cat([_to_dev(t, dev) for t in labels_h]).contiguous()
        tab, lsa_tab = tabs[:8 * B].view(B, 8), tabs[8 * B:].view(B, 4)

        # ---- matching: one point set per image, the cost blocks, B assignments, targets ----
        assign = points.get("assign")
        if assign is None:
            pts_a = f32(B * self.num_points * 2)
            hip.uniform(pts_a, seed, rank, step, hip.TRI_SITE_ASSIGN)
            pts_a = pts_a.view(B, self.num_points, 2)
        else:
            if len(assign) != B:
                raise ValueError("points['assign']: one [Np, 2] per image (%d)" % B)
            pts_a = torch.stack([_to_dev(torch.as_tensor(p).reshape(-1, 2), dev).to(torch.float32)
                                 for p in assign]).contiguous()
        cost = f32(c_off)
        scratch = hip.tri_match_cost(sub, obj, rel, s_seg, o_seg, gt_all, pts_a, gt_rels, gl, tab,
                                     self.cost_weights, max(G), Q * max(R), cost)
        rows, cols = i32(o_off), i32(o_off)
        lsa_status = torch.zeros(B, device=dev, dtype=torch.int32)
        self.last_on_device = max([Q] + R) <= hip.LSA_MAX_SIDE
        if self.last_on_device:
            hip.lsa(cost, lsa_tab, rows, cols, lsa_status, max_cells=Q * max(R))
        else:
            host = cost.cpu().numpy()
            r_h, c_h = np.zeros(o_off, np.int32), np.zeros(o_off, np.int32)
            co = po = 0
            for b in range(B):
                r, c = linear_sum_assignment(host[co:co + Q * R[b]].reshape(Q, R[b]))
                order = np.argsort(r)
                r_h[po:po + P_b[b]], c_h[po:po + P_b[b]] = r[order], c[order]
                co, po = co + Q * R[b], po + P_b[b]
            rows, cols = torch.from_numpy(r_h).to(dev), torch.from_numpy(c_h).to(dev)
        labels = torch.empty(3, B * Q, device=dev, dtype=torch.int64)
        matched = torch.full((M, 4), -1, device=dev, dtype=torch.int64)
        side_rows = torch.full((2, M, 4), -1, device=dev, dtype=torch.int64)
        rel_idx = torch.full((M,), -1, device=dev, dtype=torch.int64)
        mcount, status = i32(1), i32(1)
        hip.tri_targets(tab, rows, cols, lsa_status, gt_rels, gl, Q, self.num_classes,
                        self.num_relations, labels, matched, side_rows, rel_idx, mcount, status)
        self.assign_status = status
        self.last = dict(sub_labels=labels[0], obj_labels=labels[1], rel_labels=labels[2],
                         matched=matched, rel_idx=rel_idx, mcount=mcount, counts=list(P_b))
        if debug:
            self.last.update(cost=cost, rows=rows, cols=cols, lsa_status=lsa_status, assign=pts_a,
                             tab=tab, gt_rels=gt_rels, scratch=scratch)

        # ---- the three class terms ----
        if self._cw is None or self._cw[0].device != dev:
            self._cw = [torch.tensor(v, dtype=torch.float32, device=dev) for v in
                        (self.sub_class_weight, self.obj_class_weight, self.rel_class_weight)]
        out_cls = f32(3)
        g_cls = []
        for i, x in enumerate((sub, obj, rel)):
            x3, y2 = x.view(1, B * Q, -1), labels[i].view(1, B * Q)
            hip.ce_avg(x3, y2, self._cw[i], out_cls[i:i + 1], self.w_cls[i])
            if grads is not None:
                g = torch.empty_like(x3)
                hip.ce_avg_grad(x3, y2, self._cw[i], g, self.w_cls[i])
                g_cls.append(g.view(1, B, Q, -1))

        # ---- the mask and dice terms of each side over its matched rows' loss points ----
        ok = matched[:, 0] >= 0
        idx_pred = torch.where(ok, matched[:, 0] * Q + matched[:, 1], matched[:, 0])
        out_m, g_mask = [], []
        ntm = 0.0 if num_total_masks is None else float(num_total_masks)
        # (both sides' mask gradients are the halves of ONE buffer: `PSGTr2HeadGrad.backward` reads
        # them as the [2 M, h * w] operand of the mask products without a copy)
        g_both = f32(2, M, h, w) if grads is not None else None
        sites = ((hip.TRI_SITE_SUB_CANDIDATES, hip.TRI_SITE_SUB_TAIL),
                 (hip.TRI_SITE_OBJ_CANDIDATES, hip.TRI_SITE_OBJ_TAIL))
        for s, (name, maps) in enumerate((("sub", s_seg), ("obj", o_seg))):
            maps = maps.view(B * Q, h, w)
            srows = side_rows[s]
            idx_gt = srows[:, 3].contiguous()
            as_pts = lambda t: _to_dev(torch.as_tensor(t), dev).to(torch.float32).reshape(M, -1, 2) \
                .contiguous()
            if name + "_loss" in points:
                pts = as_pts(points[name + "_loss"])
                Np = pts.shape[1]
            else:
                Np = self.num_points
                S = int(Np * self.oversample_ratio)
                k = int(self.importance_sample_ratio * Np)
                if name + "_candidates" in points:
                    cand = as_pts(points[name + "_candidates"])
                else:
                    cand = f32(M * S * 2)
                    hip.uniform(cand, seed, rank, step, sites[s][0])
                    cand = cand.view(M, S, 2)
                tail = None
                if k < Np and name + "_tail" in points:
                    tail = as_pts(points[name + "_tail"])
                elif k < Np:
                    tail = f32(M * (Np - k) * 2)
                    hip.uniform(tail, seed, rank, step, sites[s][1])
                    tail = tail.view(M, Np - k, 2)
                if cand.shape != (M, S, 2) or (tail is not None and tail.shape != (M, Np - k, 2)):
                    raise ValueError("points: %s_candidates [%d, %d, 2] and %s_tail [%d, %d, 2]"
                                     % (name, M, S, name, M, Np - k))
                keys, pts = i32(M, S), f32(M, Np, 2)
                hip.uncertain_points(maps, srows, B, Q, cand, tail, k, keys, pts)
                if debug:
                    self.last.update({name + "_keys": keys, name + "_candidates": cand, "k": k})
            x, t = f32(M, Np), f32(M, Np)
            hip.point_sample_rows(maps, idx_pred, pts, x)
            hip.point_sample_rows(gt_all, idx_gt, pts, t)
            o4, sums = f32(4), f32(M, 4)
            coef = f32(M, Np) if grads is not None else None
            hip.mask_point_loss(x, t, srows, 1, self.w_mask[s], self.w_dice[s], self.dice_eps[s],
                                sums, o4, coef, ntm)
            out_m.append(o4)
            if debug:
                self.last.update({name + "_points": pts, name + "_x": x, name + "_t": t,
                                  name + "_sums": sums, name + "_coef": coef})
            if grads is not None:
                g = g_both[s]
                scr = i32(hip.point_scatter_scratch_ints(M, Np, h, w))
                hip.point_scatter_grad(coef, pts, g, scr)
                g_mask.append(g)
        if grads is not None:
            grads.update(sub=g_cls[0], obj=g_cls[1], rel=g_cls[2], mask_rows=idx_pred,
                         sub_mask=g_mask[0], obj_mask=g_mask[1])
        return dict(s_loss_cls=out_cls[0], o_loss_cls=out_cls[1], r_loss_cls=out_cls[2],
                    s_loss_mask=out_m[0][0], o_loss_mask=out_m[1][0],
                    s_loss_dice=out_m[0][1], o_loss_dice=out_m[1][1])
