"""Loss of `CrossHeadBBox` on device outputs: the reference's `CrossHeadBBox.loss`
(pairnet/models/relation_heads/pairnet_bbox_head.py:362-464, `loss_single` :546-704,
`_get_target_single` :848-966) under configs/deformable_detr/cross_r101_vg.py:122-164.

The reference has its detection terms commented out (:362-464, :596-642); what is left is
`CrossHead2.loss` with ONE other piece: the object assignment that says which of the 100 kept
queries stands for which ground-truth box is [3P] mmdet's `HungarianAssigner` on
FocalLossCost + BBoxL1Cost(xywh) + IoUCost(giou) (:863-865) instead of the mask assigner.  So
`CrossHeadBBoxLoss` is `CrossHead2Loss` (losses.py) with that cost: `pn_box_match_cost_f32`
(csrc/box_loss.hip) writes every image's 100 x G block in one launch; the id-matcher cost
(`pn_id_match_cost_f32`), the `pn_lsa_f32` solve, `pn_loss_targets` and the four reductions with
their logit gradients (`_reduce`) are the parent's, unchanged.

  host mode (default)   scipy on the downloaded cost blocks, where the reference solves them
                        (`linear_sum_assignment(cost.cpu())`); a NaN cost raises as scipy does.
  device_targets=True   no host wait: costs -> ONE pn_lsa_f32 launch over the 2B problems ->
                        pn_loss_targets; `assign_status` (device int32 [1]) is non-zero where the
                        host path would have raised, and the targets keep their fills.

Quirks kept: an unmatched ground-truth box points at query 1 (`torch.ones_like`, :888-890); the
importance target is 1 at each ground-truth (subject query, object query) pair, duplicates
included, on the literal 100 x 100 grid (:902-903); an image without ground-truth relations is a
ValueError (the reference fails on it with an AttributeError).

`loss_r_cls`.  The live line :689 hands SeesawLoss the C relation logits alone, which [3P] mmdet's
SeesawLoss (C + 2 columns, a dict with `return_dict=True`) does not accept: under the shipped config
that line cannot run.  What is computed here is SeesawLoss's class part over the C relation classes
-- the commented-out lines :684-687 (two dummy objectness columns appended,
`["loss_cls_classes"]`), which is also what `CrossHead2.loss` computes (pairnet_head.py:529-536).
tests/bbox_loss_ref.py runs the reference method in place with exactly that adapter.
"""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import hip
from .config import ConfigDict
from .losses import CrossHead2Loss, _to_dev

_MASK_DEFAULTS = dict(
    mask_assigner=dict(type="MaskHungarianAssigner",
                       cls_cost=dict(type="ClassificationCost", weight=2.0),
                       mask_cost=dict(type="CrossEntropyLossCost", weight=5.0, use_sigmoid=True),
                       dice_cost=dict(type="DiceCost", weight=5.0, pred_act=True, eps=1.0)))


class CrossHeadBBoxLoss(CrossHead2Loss):
    KEPT = 100          # the literal 100 of pairnet_bbox_head.py:902

    def __init__(self, num_classes, num_relations, num_rel_query=100, train_cfg=None,
                 rel_cls_loss=None, subobj_cls_loss=None, importance_match_loss=None):
        t = ConfigDict(train_cfg or dict(
            id_assigner=dict(type="IdMatcher", sub_id_cost=dict(type="ClassificationCost", weight=1.0),
                             obj_id_cost=dict(type="ClassificationCost", weight=1.0),
                             r_cls_cost=dict(type="ClassificationCost", weight=0.0)),
            bbox_assigner=dict(type="HungarianAssigner",
                               cls_cost=dict(type="FocalLossCost", weight=2.0),
                               reg_cost=dict(type="BBoxL1Cost", weight=5.0, box_format="xywh"),
                               iou_cost=dict(type="IoUCost", iou_mode="giou", weight=2.0)),
            sampler=dict(type="PseudoSampler")))
        ba = t["bbox_assigner"]
        want = [(ba["type"], "HungarianAssigner"), (ba["cls_cost"]["type"], "FocalLossCost"),
                (ba["reg_cost"]["type"], "BBoxL1Cost"), (ba["iou_cost"]["type"], "IoUCost"),
                (t.get("sampler", dict(type="PseudoSampler"))["type"], "PseudoSampler")]
        for got, exp in want:
            if got != exp:
                raise NotImplementedError("%s (built: %s, configs/deformable_detr/cross_r101_vg.py:"
                                          "151-165)" % (got, exp))
        if ba["reg_cost"].get("box_format", "xyxy") != "xywh" \
                or ba["iou_cost"].get("iou_mode", "giou") != "giou" \
                or ba["cls_cost"].get("binary_input", False):
            raise NotImplementedError("BBoxL1Cost(box_format='xywh'), IoUCost(iou_mode='giou'), "
                                      "FocalLossCost on class logits")
        # (the parent checks the id assigner and the three losses; its mask assigner is not used)
        super().__init__(num_classes, num_relations, self.KEPT, num_rel_query,
                         train_cfg=dict(_MASK_DEFAULTS, id_assigner=t["id_assigner"],
                                        sampler=dict(type="MaskPseudoSampler")),
                         rel_cls_loss=rel_cls_loss, subobj_cls_loss=subobj_cls_loss,
                         importance_match_loss=importance_match_loss)
        cc = ba["cls_cost"]
        self.box_w = (float(cc.get("weight", 1.0)), float(ba["reg_cost"].get("weight", 1.0)),
                      float(ba["iou_cost"].get("weight", 1.0)))
        self.focal = dict(alpha=float(cc.get("alpha", 0.25)), gamma=float(cc.get("gamma", 2.0)),
                          eps=float(cc.get("eps", 1e-12)))

    # ---- the batch's sizes, tables and ground truth: host work from shapes alone ----
    def _prepare(self, B, gt_rels_list, gt_bboxes_list, gt_labels_list, img_metas, dev):
        Q, R = self.Q, self.R
        pieces, boxes, lsa_tab, tgt_tab, box_tab, where = [], [], [], [], [], []
        c_off = o_off = g_off = b_off = 0
        for i in range(B):
            rels, gl = self._gt_tensors(gt_rels_list[i], gt_labels_list[i])
            gb = torch.as_tensor(gt_bboxes_list[i]).reshape(-1, 4).to(torch.float32)
            T, G = rels.shape[0], gl.shape[0]
            if gb.shape[0] != G:
                raise ValueError("image %d: %d labels for %d boxes" % (i, G, gb.shape[0]))
            if G == 0:
                raise ValueError("an image without ground-truth boxes cannot carry relations")
            if rels.device != gl.device:
                rels, gl = _to_dev(rels, dev), _to_dev(gl, dev)
            s_o = rels[:, :2].clamp(0, G - 1) if rels.is_cuda else rels[:, :2]
            pieces += [gl, rels.reshape(-1), gl[s_o[:, 0]], gl[s_o[:, 1]], rels[:, 2] - 1]
            boxes.append(gb)
            where.append(dict(G=G, T=T, gl=g_off, sub=g_off + G + 3 * T, obj=g_off + G + 4 * T,
                              rel=g_off + G + 5 * T, cost=c_off, cost2=c_off + Q * G, out=o_off,
                              out2=o_off + min(Q, G)))
            lsa_tab += [c_off, Q, G, o_off, c_off + Q * G, R, T, o_off + min(Q, G)]
            tgt_tab += [g_off, g_off + G, G, T]
            box_tab += [c_off, G, g_off, b_off]
            c_off += Q * G + R * T
            o_off += min(Q, G) + min(R, T)
            g_off += G + 6 * T
            b_off += G
        for m in img_metas:          # factor = (img_w, img_h, img_w, img_h) of `img_shape`
            h, w = m["img_shape"][:2]
            boxes.append(torch.tensor([[w, h, w, h]], dtype=torch.float32))
        head = torch.tensor(lsa_tab + tgt_tab + box_tab, dtype=torch.int64)
        nh = head.numel()
        # ---- two pinned, non-blocking uploads: (tables + integer ground truth), (boxes + factors) ----
        if all(not p.is_cuda for p in pieces):
            buf = torch.empty(nh + g_off, dtype=torch.int64, pin_memory=True)
            torch.cat([head] + pieces, out=buf)
            up = buf.to(dev, non_blocking=True)
            tabs, gt = up[:nh], up[nh:]
        else:
            tabs, gt = _to_dev(head, dev), torch.cat([_to_dev(p, dev) for p in pieces])
        if all(not b.is_cuda for b in boxes):
            fb = torch.empty(b_off + B, 4, dtype=torch.float32, pin_memory=True)
            torch.cat(boxes, out=fb)
            fb = fb.to(dev, non_blocking=True)
        else:
            fb = torch.cat([_to_dev(b, dev) for b in boxes])
        return dict(where=where, lsa_tab=tabs[:8 * B].view(2 * B, 4),
                    tgt_tab=tabs[8 * B:12 * B].view(B, 4), box_tab=tabs[12 * B:].view(B, 4), gt=gt,
                    gt_boxes=fb[:b_off], factor=fb[b_off:], cost_len=c_off, out_len=o_off)

    def _costs(self, cls, box, sub, obj, rel, p):
        """Every cost block of the batch: the box costs in ONE launch, the id costs per image."""
        Q, R, dev = self.Q, self.R, cls.device
        cost_all = torch.empty(p["cost_len"], device=dev, dtype=torch.float32)
        hip.box_match_cost(cls.contiguous(), box.contiguous(), p["gt"], p["gt_boxes"], p["factor"],
                           p["box_tab"], cost_all, max(Q * w["G"] for w in p["where"]),
                           *self.box_w, **self.focal)
        gt = p["gt"]
        for i, w in enumerate(p["where"]):
            T = w["T"]
            cost2 = cost_all[w["cost2"]:w["cost2"] + R * T].view(R, T)
            hip.id_match_cost(sub[i].contiguous(), obj[i].contiguous(), rel[i].contiguous(),
                              gt[w["sub"]:w["sub"] + T], gt[w["obj"]:w["obj"] + T],
                              gt[w["rel"]:w["rel"] + T], cost2, *self.id_w)
        return cost_all

    @torch.no_grad()
    @hip.on_device
    def loss(self, all_cls_scores, all_bbox_preds, gt_rels_list, gt_bboxes_list, gt_labels_list,
             img_metas, gt_bboxes_ignore=None, trace=None, grads=None, device_targets=False):
        """The reference's signature (pairnet_bbox_head.py:362-371) -> its four keys as 0-dim device
        tensors; `grads={}` receives d (their sum) / d logits for "obj", "sub", "rel", "importance";
        `trace=[]` receives per image the assignments and cost blocks (synchronises).
        `device_targets`: build the targets on the device without a host wait (module docstring)."""
        assert gt_bboxes_ignore is None, "Only supports for gt_bboxes_ignore setting to None."
        cls, sub, obj = all_cls_scores["cls"], all_cls_scores["sub"], all_cls_scores["obj"]
        rel, imp, box = all_cls_scores["rel"], all_cls_scores["importance"], all_bbox_preds["bbox"]
        B, dev, Q, R = cls.shape[0], cls.device, self.Q, self.R
        if cls.shape[1] != Q or tuple(box.shape) != (B, Q, 4) or tuple(imp.shape) != (B, Q, Q):
            raise ValueError("the loss is written for the %d kept queries (pairnet_bbox_head.py:902)"
                             % Q)
        if len(img_metas) != B:
            raise ValueError("%d img_metas for a batch of %d" % (len(img_metas), B))
        p = self._prepare(B, gt_rels_list, gt_bboxes_list, gt_labels_list, img_metas, dev)
        if not self._fits_device(gt_rels_list, gt_labels_list):
            raise NotImplementedError("at most %d boxes / relations per image" % hip.LSA_MAX_SIDE)
        cost_all = self._costs(cls, box, sub, obj, rel, p)
        self.last_on_device = bool(device_targets)
        where = p["where"]
        if self.last_on_device:
            i32 = lambda n: torch.empty(n, device=dev, dtype=torch.int32)
            rows, cols = i32(p["out_len"]), i32(p["out_len"])
            status, bstatus = i32(2 * B), i32(1)
            hip.lsa(cost_all, p["lsa_tab"], rows, cols, status,
                    max_cells=max(max(Q * w["G"], R * w["T"]) for w in where))
            importance = torch.empty(B, Q, Q, device=dev, dtype=torch.float32)
            labels = torch.empty(3, B * R, device=dev, dtype=torch.int64)
            cum = self._cum_on(dev)
            hip.loss_targets(p["lsa_tab"], rows, cols, status, p["tgt_tab"], p["gt"], Q, R,
                             importance, labels, cum, bstatus)
            self.assign_status = bstatus
            if trace is not None:           # (a debugging aid: this part synchronises)
                h = lambda t: t.cpu().numpy().astype(np.int64)
                for w in where:
                    n1, n2 = min(Q, w["G"]), min(R, w["T"])
                    trace.append(dict(
                        box_rows=h(rows[w["out"]:w["out"] + n1]),
                        box_cols=h(cols[w["out"]:w["out"] + n1]),
                        triplet_rows=h(rows[w["out2"]:w["out2"] + n2]),
                        triplet_cols=h(cols[w["out2"]:w["out2"] + n2]),
                        box_cost=cost_all[w["cost"]:w["cost"] + Q * w["G"]].view(Q, -1).cpu(),
                        id_cost=cost_all[w["cost2"]:w["cost2"] + R * w["T"]].view(R, -1).cpu()))
            tgt = dict(o=labels[2], s=labels[1], r=labels[0], cum=cum[:self.num_relations],
                       imp=importance)
            return self._reduce(obj, sub, rel, imp, tgt.__getitem__, grads)
        # ---- host mode: scipy on the downloaded blocks, the bookkeeping of :888-951 on the host ----
        cost_host = cost_all.cpu().numpy()
        r_lab, s_ids, o_ids, gt_imp = [], [], [], []
        for i, w in enumerate(where):
            G, T = w["G"], w["T"]
            gt_rels = np.asarray(torch.as_tensor(gt_rels_list[i]).cpu()).reshape(-1, 3).astype(np.int64)
            gl = np.asarray(torch.as_tensor(gt_labels_list[i]).cpu()).astype(np.int64).reshape(-1)
            cost = cost_host[w["cost"]:w["cost"] + Q * G].reshape(Q, G)
            cost2 = cost_host[w["cost2"]:w["cost2"] + R * T].reshape(R, T)
            rows, cols = linear_sum_assignment(cost)                    # (host, as the reference)
            query_of_gt = np.ones(G, dtype=np.int64)
            order = np.argsort(rows)          # PseudoSampler: positives in ascending query order
            query_of_gt[cols[order]] = rows[order]
            gt_rel = gt_rels[:, 2] - 1
            gt_sub_cls, gt_obj_cls = gl[gt_rels[:, 0]], gl[gt_rels[:, 1]]
            importance = np.zeros((Q, Q), dtype=np.float32)
            importance[query_of_gt[gt_rels[:, 0]], query_of_gt[gt_rels[:, 1]]] = 1.0
            rows2, cols2 = linear_sum_assignment(cost2)
            r_labels = np.full(R, -1, dtype=np.int64)
            sub_ids, obj_ids = r_labels.copy(), r_labels.copy()
            r_labels[rows2], sub_ids[rows2], obj_ids[rows2] = \
                gt_rel[cols2], gt_sub_cls[cols2], gt_obj_cls[cols2]
            if trace is not None:
                trace.append(dict(box_rows=rows, box_cols=cols, triplet_rows=rows2,
                                  triplet_cols=cols2, box_cost=torch.from_numpy(cost.copy()),
                                  id_cost=torch.from_numpy(cost2.copy())))
            for lst, v in zip((r_lab, s_ids, o_ids, gt_imp), (r_labels, sub_ids, obj_ids, importance)):
                lst.append(v)
        r_lab, s_ids, o_ids = (np.concatenate(x) for x in (r_lab, s_ids, o_ids))
        np.add.at(self.cum_samples, r_lab[r_lab >= 0], 1.0)   # SeesawLoss counts before it weighs
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        host = dict(o=o_ids, s=s_ids, r=r_lab, imp=np.stack(gt_imp, 0))
        get = lambda k: up(self.cum_samples[:self.num_relations]) if k == "cum" else up(host[k])
        return self._reduce(obj, sub, rel, imp, get, grads)
