"""Reference statements for the box head's loss (pair-net_amd/bbox_losses.py, csrc/box_loss.hip).

FROM MEMORY, UNPINNED: mmdet is not installed where this project is built, so the [3P] pieces the
reference's `CrossHeadBBox.loss` calls -- `FocalLossCost`, `BBoxL1Cost`, `IoUCost` (with
`bbox_overlaps`), `HungarianAssigner`, `PseudoSampler` / `SamplingResult` (mmdet 2.x,
mmdet/core/bbox/{match_costs,assigners,samplers,iou_calculators}) -- are restated here from memory.
Nothing pins them to mmdet's own code (INTEGRATION.md lists them among the unpinned restatements).
They run in whatever dtype their inputs have: float64 is the reference the GPU tests compare
against, fp32 gives the rounding a torch implementation of the same formulas shows.

What IS pinned: `targets_single` / `loss` below restate the reference's own `_get_target_single` /
`loss_single` (pairnet_bbox_head.py:848-966, :546-704), and tests/test_bbox_loss_refs.py runs the
reference's `CrossHeadBBox.loss` in place (through oracle/ref_shim, with these restated assigner and
sampler patched onto the loaded module) and requires agreement to 1e-12 in float64.

`loss_r_cls`: the live line pairnet_bbox_head.py:689 hands SeesawLoss the C relation logits alone;
mmdet's SeesawLoss takes C + 2 columns and (with the config's `return_dict=True`) returns a dict, so
under the shipped config that line cannot run.  `SeesawClassPart` is the adapter under which it is
run here: the two dummy objectness columns appended and `["loss_cls_classes"]` taken -- the
reference's commented-out lines :684-687, and what `CrossHead2.loss` does (pairnet_head.py:529-536).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import mmdet_train as T   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bbox_loss.npz")
CFG = dict(w_cls=2.0, w_reg=5.0, w_iou=2.0, alpha=0.25, gamma=2.0, eps=1e-12, iou_eps=1e-6)
KEPT = 100


# ------------------------------------------------------------ [3P] restated, from memory, unpinned
def bbox_cxcywh_to_xyxy(b):
    cx, cy, w, h = b.split((1, 1, 1, 1), dim=-1)
    return torch.cat([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)


def bbox_xyxy_to_cxcywh(b):
    x1, y1, x2, y2 = b.split((1, 1, 1, 1), dim=-1)
    return torch.cat([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1], dim=-1)


def giou_parts(b1, b2, eps=1e-6):
    """mmdet bbox_overlaps(mode="giou", is_aligned=False) -> (gious [n, m], overlap, union,
    enclose_area); union and enclosing area clamped to >= eps."""
    area1 = (b1[..., 2] - b1[..., 0]) * (b1[..., 3] - b1[..., 1])
    area2 = (b2[..., 2] - b2[..., 0]) * (b2[..., 3] - b2[..., 1])
    lt = torch.max(b1[..., :, None, :2], b2[..., None, :, :2])
    rb = torch.min(b1[..., :, None, 2:], b2[..., None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = area1[..., None] + area2[..., None, :] - overlap
    e_lt = torch.min(b1[..., :, None, :2], b2[..., None, :, :2])
    e_rb = torch.max(b1[..., :, None, 2:], b2[..., None, :, 2:])
    eps = union.new_tensor([eps])
    union = torch.max(union, eps)
    ious = overlap / union
    e_wh = (e_rb - e_lt).clamp(min=0)
    enclose = torch.max(e_wh[..., 0] * e_wh[..., 1], eps)
    return ious - (enclose - union) / enclose, overlap, union, enclose


@T.MATCH_COST.register_module()
class FocalLossCost:
    """mmdet match_cost.FocalLossCost (binary_input=False)."""

    def __init__(self, weight=1.0, alpha=0.25, gamma=2, eps=1e-12, binary_input=False):
        assert not binary_input
        self.weight, self.alpha, self.gamma, self.eps = weight, alpha, gamma, eps

    def __call__(self, cls_pred, gt_labels):
        cls_pred = cls_pred.sigmoid()
        neg_cost = -(1 - cls_pred + self.eps).log() * (1 - self.alpha) * cls_pred.pow(self.gamma)
        pos_cost = -(cls_pred + self.eps).log() * self.alpha * (1 - cls_pred).pow(self.gamma)
        return (pos_cost[:, gt_labels] - neg_cost[:, gt_labels]) * self.weight


@T.MATCH_COST.register_module()
class BBoxL1Cost:
    """mmdet match_cost.BBoxL1Cost: L1 distance of normalised boxes (cdist, p = 1)."""

    def __init__(self, weight=1.0, box_format="xyxy"):
        assert box_format in ("xyxy", "xywh")
        self.weight, self.box_format = weight, box_format

    def __call__(self, bbox_pred, gt_bboxes):
        if self.box_format == "xywh":
            gt_bboxes = bbox_xyxy_to_cxcywh(gt_bboxes)
        else:
            bbox_pred = bbox_cxcywh_to_xyxy(bbox_pred)
        return torch.cdist(bbox_pred, gt_bboxes, p=1) * self.weight


@T.MATCH_COST.register_module()
class IoUCost:
    """mmdet match_cost.IoUCost."""

    def __init__(self, iou_mode="giou", weight=1.0):
        assert iou_mode == "giou"
        self.weight, self.iou_mode = weight, iou_mode

    def __call__(self, bboxes, gt_bboxes):
        return -giou_parts(bboxes, gt_bboxes)[0] * self.weight


@T.BBOX_ASSIGNERS.register_module()
class HungarianAssigner(T.BaseAssigner):
    """mmdet HungarianAssigner.assign: classification + L1 + IoU cost, scipy on the host."""

    def __init__(self, cls_cost=dict(type="ClassificationCost", weight=1.0),
                 reg_cost=dict(type="BBoxL1Cost", weight=1.0),
                 iou_cost=dict(type="IoUCost", iou_mode="giou", weight=1.0)):
        self.cls_cost = T.build_match_cost(cls_cost)
        self.reg_cost = T.build_match_cost(reg_cost)
        self.iou_cost = T.build_match_cost(iou_cost)

    def cost(self, bbox_pred, cls_pred, gt_bboxes, gt_labels, img_meta):
        img_h, img_w, _ = img_meta["img_shape"]
        factor = gt_bboxes.new_tensor([img_w, img_h, img_w, img_h]).unsqueeze(0)
        cls_cost = self.cls_cost(cls_pred, gt_labels)
        reg_cost = self.reg_cost(bbox_pred, gt_bboxes / factor)
        bboxes = bbox_cxcywh_to_xyxy(bbox_pred) * factor
        iou_cost = self.iou_cost(bboxes, gt_bboxes)
        return cls_cost + reg_cost + iou_cost

    def assign(self, bbox_pred, cls_pred, gt_bboxes, gt_labels, img_meta, gt_bboxes_ignore=None,
               eps=1e-7):
        assert gt_bboxes_ignore is None
        num_gts, num_bboxes = gt_bboxes.size(0), bbox_pred.size(0)
        assigned_gt_inds = bbox_pred.new_full((num_bboxes,), -1, dtype=torch.long)
        assigned_labels = bbox_pred.new_full((num_bboxes,), -1, dtype=torch.long)
        if num_gts == 0 or num_bboxes == 0:
            if num_gts == 0:
                assigned_gt_inds[:] = 0
            return T.AssignResult(num_gts, assigned_gt_inds, None, labels=assigned_labels)
        cost = self.cost(bbox_pred, cls_pred, gt_bboxes, gt_labels, img_meta).detach().cpu()
        self.last_cost = cost
        rows, cols = linear_sum_assignment(cost)
        rows = torch.from_numpy(rows).to(bbox_pred.device)
        cols = torch.from_numpy(cols).to(bbox_pred.device)
        assigned_gt_inds[:] = 0
        assigned_gt_inds[rows] = cols + 1
        assigned_labels[rows] = gt_labels[cols]
        return T.AssignResult(num_gts, assigned_gt_inds, None, labels=assigned_labels)


class SamplingResult:
    """mmdet SamplingResult (the fields pairnet_bbox_head.py:867-951 reads)."""

    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.pos_is_gt = gt_flags[pos_inds]
        self.num_gts = gt_bboxes.shape[0]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        if gt_bboxes.numel() == 0:
            self.pos_gt_bboxes = torch.empty_like(gt_bboxes).view(-1, 4)
        else:
            if len(gt_bboxes.shape) < 2:
                gt_bboxes = gt_bboxes.view(-1, 4)
            self.pos_gt_bboxes = gt_bboxes[self.pos_assigned_gt_inds.long(), :]
        self.pos_gt_labels = assign_result.labels[pos_inds] if assign_result.labels is not None \
            else None


@T.BBOX_SAMPLERS.register_module()
class PseudoSampler:
    """mmdet PseudoSampler: every assigned query is a positive sample, in ascending order."""

    def __init__(self, **kwargs):
        pass

    def sample(self, assign_result, bboxes, gt_bboxes, *args, **kwargs):
        pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        gt_flags = bboxes.new_zeros(bboxes.shape[0], dtype=torch.uint8)
        return SamplingResult(pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags)


class SeesawClassPart(T.SeesawLoss):
    """The adapter of the module docstring: SeesawLoss's class part on C logits."""

    def forward(self, cls_score, labels, *a, **kw):
        dummy = cls_score.new_zeros((cls_score.shape[0], 2))
        return super().forward(torch.cat([cls_score, dummy], dim=1), labels, *a, **kw)[
            "loss_cls_classes"]


# --------------------------------------------------------- the cost, cell by cell, with magnitudes
def cost_terms(cls, box, gt_labels, gt_bboxes, factor, dtype=torch.float64, cfg=CFG):
    """One image's [Q, G] cost in `dtype` from fp32 data, as `HungarianAssigner.cost` forms it, and
    the per-cell MAGNITUDE the GPU bound is relative to: |cls terms| (with the conditioning of
    `1 - p`, below) + |reg terms| + the GIoU's
    intermediates (both areas, overlap, union, enclosing area, each divided by the area it is
    divided by, times w_iou) -- so that the cancellation in `enclose - union` and in
    `area1 + area2 - overlap` is covered.  factor: [4] = (w, h, w, h)."""
    c = {k: v for k, v in cfg.items()}
    cls, box, gt, f = cls.to(dtype), box.to(dtype), gt_bboxes.to(dtype), factor.to(dtype).view(1, 4)
    p = cls.sigmoid()
    neg = -(1 - p + c["eps"]).log() * (1 - c["alpha"]) * p.pow(c["gamma"])
    pos = -(p + c["eps"]).log() * c["alpha"] * (1 - p).pow(c["gamma"])
    cls_cost = (pos[:, gt_labels] - neg[:, gt_labels]) * c["w_cls"]
    gt_c = bbox_xyxy_to_cxcywh(gt / f)
    diffs = (box[:, None, :] - gt_c[None, :, :]).abs()
    reg_cost = torch.cdist(box, gt_c, p=1) * c["w_reg"]
    boxes = bbox_cxcywh_to_xyxy(box) * f
    giou, overlap, union, enclose = giou_parts(boxes, gt, c["iou_eps"])
    iou_cost = -giou * c["w_iou"]
    cost = cls_cost + reg_cost + iou_cost
    area1 = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).abs()[:, None]
    area2 = ((gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])).abs()[None, :]
    # the coordinates the areas are differences of: their rounding enters the areas relative to the
    # products of the coordinates, not of the sides
    ext1 = (boxes[:, 2].abs() + boxes[:, 0].abs()) * (boxes[:, 3].abs() + boxes[:, 1].abs())
    ext2 = (gt[:, 2].abs() + gt[:, 0].abs()) * (gt[:, 3].abs() + gt[:, 1].abs())
    ext = ext1[:, None] + ext2[None, :]
    inter = (area1 + area2 + overlap + union + ext) / union + (enclose + union + ext) / enclose \
        + overlap / union
    # the focal terms' conditioning: p = sigmoid(x) is rounded to 2^-24 p, and `1 - p` hands that
    # ABSOLUTE error to log(1 - p + eps) (divided by its argument) and to (1 - p)^gamma -- the
    # formula's own cancellation for a confident logit, in any fp32 evaluation of it
    a, ga, e = c["alpha"], c["gamma"], c["eps"]
    q1 = 1 - p
    m_neg = ((q1 + e).log().abs() + p / (q1 + e)) * (1 - a) * p.pow(ga)
    m_pos = ((p + e).log().abs() * (q1.pow(ga) + ga * p * q1.pow(ga - 1))
             + p / (p + e) * q1.pow(ga)) * a
    mag = (m_pos[:, gt_labels] + m_neg[:, gt_labels]) * c["w_cls"] \
        + (diffs.sum(-1) + box.abs().sum(-1)[:, None] + gt_c.abs().sum(-1)[None, :]) * c["w_reg"] \
        + inter * c["w_iou"]
    return cost, mag


# ----------------------------------------- the reference's own target / loss code, restated (pinned)
def build_parts(num_classes, num_relations, cum=None):
    assigner = HungarianAssigner(cls_cost=dict(type="FocalLossCost", weight=CFG["w_cls"]),
                                 reg_cost=dict(type="BBoxL1Cost", weight=CFG["w_reg"],
                                               box_format="xywh"),
                                 iou_cost=dict(type="IoUCost", iou_mode="giou", weight=CFG["w_iou"]))
    rel_loss = SeesawClassPart(num_classes=num_relations, return_dict=True, loss_weight=2.0)
    if cum is not None:
        rel_loss.cum_samples.copy_(torch.as_tensor(cum))
    so = T.CrossEntropyLoss(use_sigmoid=False, loss_weight=4.0, reduction="mean",
                            class_weight=[1.0] * num_classes)
    return assigner, PseudoSampler(), rel_loss, so


def id_match(sub, obj, rel, gt_sub, gt_obj, gt_rel, w=(1.0, 1.0, 0.0)):
    """IdMatcher.assign (approaches/matcher.py:219-274) -> (gt_inds, cost)."""
    n = rel.shape[0]
    gt_inds = rel.new_full((n,), -1, dtype=torch.long)
    cost = (-sub.softmax(-1)[:, gt_sub] * w[0]) + (-obj.softmax(-1)[:, gt_obj] * w[1]) \
        + (-rel.softmax(-1)[:, gt_rel] * w[2])
    rows, cols = linear_sum_assignment(cost.detach().cpu())
    gt_inds[:] = 0
    gt_inds[torch.from_numpy(rows)] = torch.from_numpy(cols) + 1
    return gt_inds, cost.detach()


def margin(cost):
    """How far the optimal assignment of `cost` is from the best one that differs from it: the
    smallest increase of the total when one optimal pair is forbidden."""
    cost = np.asarray(cost, dtype=np.float64)
    rows, cols = linear_sum_assignment(cost)
    best = cost[rows, cols].sum()
    big = np.abs(cost).sum() + 1.0
    m = np.inf
    for r, c in zip(rows, cols):
        alt = cost.copy()
        alt[r, c] = big
        r2, c2 = linear_sum_assignment(alt)
        m = min(m, alt[r2, c2].sum() - best)
    return m


def targets_single(case, i, dtype, assigner, sampler):
    """pairnet_bbox_head.py:848-966 for image i of a case, in `dtype`."""
    to = lambda t: t.to(dtype)
    sub, obj, cls = to(case["sub"][i]), to(case["obj"][i]), to(case["cls"][i])
    box, rel = to(case["bbox"][i]), to(case["rel"][i])
    gt_bboxes, gt_rels, gt_labels = to(case["gt_bboxes"][i]), case["gt_rels"][i], case["gt_labels"][i]
    if gt_rels.shape[0] == 0:
        raise ValueError("an image without ground-truth relations cannot be a loss target")
    res = assigner.assign(box, cls, gt_bboxes, gt_labels, case["img_metas"][i], None)
    box_cost = assigner.last_cost
    s = sampler.sample(res, box, gt_bboxes)
    query_of_gt = torch.ones_like(gt_labels)
    query_of_gt[s.pos_assigned_gt_inds] = s.pos_inds
    rels = gt_rels.T.long()
    gt_rel = rels[2] - 1
    gt_sub_cls, gt_obj_cls = gt_labels[rels[0]], gt_labels[rels[1]]
    importance = torch.zeros((KEPT, KEPT), dtype=dtype)
    importance[query_of_gt[rels[0]], query_of_gt[rels[1]]] += 1     # (index_put: no accumulation)
    tri, id_cost = id_match(sub, obj, rel, gt_sub_cls, gt_obj_cls, gt_rel)
    pos = torch.nonzero(tri > 0, as_tuple=False).squeeze(-1).unique()
    which = tri[pos] - 1
    R = rel.shape[0]
    full = lambda v: torch.full((R,), v, dtype=torch.long)
    nc = case["num_classes"]
    sub_ids, obj_ids, r_labels = full(nc), full(nc), full(-1)
    sub_ids[pos], obj_ids[pos], r_labels[pos] = gt_sub_cls[which], gt_obj_cls[which], gt_rel[which]
    weights = gt_labels.new_zeros(R)
    weights[pos] = 1.0
    trace = dict(box_rows=s.pos_inds.numpy(), box_cols=s.pos_assigned_gt_inds.numpy(),
                 triplet_rows=pos.numpy(), triplet_cols=which.numpy(), box_cost=box_cost,
                 id_cost=id_cost, query_of_gt=query_of_gt.numpy())
    return (r_labels, weights, sub_ids, obj_ids, importance), trace


def loss(case, dtype=torch.float64, grads=False):
    """The restated `loss` / `loss_single` on a case -> (losses, trace[, gradients of their sum
    w.r.t. rel / importance / sub / obj])."""
    B = case["cls"].shape[0]
    assigner, sampler, rel_loss, so_loss = build_parts(case["num_classes"], case["num_relations"],
                                                       case.get("cum"))
    rel_loss = rel_loss.to(dtype)
    leaves = {k: case[k].to(dtype).clone().requires_grad_(grads)
              for k in ("rel", "importance", "sub", "obj")}
    per, traces = [], []
    for i in range(B):
        out, tr = targets_single(case, i, dtype, assigner, sampler)
        per.append(out)
        traces.append(tr)
    r_labels, weights, sub_ids, obj_ids, importance = (list(x) for x in zip(*per))
    keep = torch.cat(weights, 0) > 0
    loss_sub = so_loss(leaves["sub"].flatten(0, 1)[keep], torch.cat(sub_ids, 0)[keep])
    loss_obj = so_loss(leaves["obj"].flatten(0, 1)[keep], torch.cat(obj_ids, 0)[keep])
    rel = leaves["rel"].reshape(-1, case["num_relations"])
    loss_rel = rel_loss(rel[keep], torch.cat(r_labels, 0)[keep])
    gt_imp = torch.stack(importance, 0)
    # (int / int64 tensor: the quotient has torch's DEFAULT dtype in the reference; here `dtype`)
    pos_weight = torch.numel(gt_imp) / (gt_imp > 0).sum().to(dtype)
    loss_match = F.binary_cross_entropy_with_logits(
        leaves["importance"], gt_imp, pos_weight=pos_weight, reduction="mean") * 5.0
    out = dict(loss_r_cls=loss_rel, loss_sub_cls=loss_sub, loss_obj_cls=loss_obj,
               loss_match=loss_match)
    if not grads:
        return out, traces
    sum(out.values()).backward()
    g = {k: v.grad.detach() for k, v in leaves.items()}
    return {k: v.detach() for k, v in out.items()}, traces, g


def loss_magnitudes(case, traces=None):
    """The four loss values' magnitudes: tests/loss_optim_ref.py's (value, mag) statements of the
    three reductions on the restated float64 targets."""
    import loss_optim_ref as LR
    B, nc, C = case["cls"].shape[0], case["num_classes"], case["num_relations"]
    assigner, sampler, _, _ = build_parts(nc, C)
    per = [targets_single(case, i, torch.float64, assigner, sampler)[0] for i in range(B)]
    r_labels, weights, sub_ids, obj_ids, importance = (list(x) for x in zip(*per))
    keep = torch.cat(weights, 0) > 0
    tgt = lambda ids: torch.where(keep, torch.cat(ids, 0), torch.full_like(keep, -1, dtype=torch.long))
    cw = torch.ones(nc, dtype=torch.float32)
    r = tgt(r_labels)
    cum = torch.as_tensor(case.get("cum", np.zeros(C + 1, np.float32))).float().clone()
    cum.index_add_(0, r[r >= 0], torch.ones(int((r >= 0).sum())))
    return dict(loss_sub_cls=float(LR.ce_mean(case["sub"].reshape(-1, nc), tgt(sub_ids), cw, 4.0)[1]),
                loss_obj_cls=float(LR.ce_mean(case["obj"].reshape(-1, nc), tgt(obj_ids), cw, 4.0)[1]),
                loss_r_cls=float(LR.seesaw_mean(case["rel"].reshape(-1, C), r, cum[:C], 0.8, 2.0,
                                                1e-2, 2.0)[1]),
                loss_match=float(LR.bce_posw_mean(case["importance"], torch.stack(importance, 0),
                                                  5.0)[1]))


# ------------------------------------------------------------------------------------- cases
def make_case(seed, G=(3, 7), T=(2, 9), num_classes=11, num_relations=7, R=100, shapes=None,
              batch_shape=(64, 80), planted=True):
    """A batch of fp32 head outputs and ground truth.  `planted`: every ground-truth box has one
    kept query sitting near it with a high logit for its label, so that the assignment has a clear
    margin; the rest of the queries are random boxes with low logits."""
    g = torch.Generator().manual_seed(seed)
    B = len(G)
    shapes = shapes or [batch_shape] * B
    rnd = lambda *s: torch.rand(*s, generator=g)
    cls = torch.randn(B, KEPT, num_classes, generator=g) - 3.0
    cxcy, wh = rnd(B, KEPT, 2) * 0.8 + 0.1, rnd(B, KEPT, 2) * 0.3 + 0.02
    bbox = torch.cat([cxcy, wh], -1)
    gt_bboxes, gt_labels, gt_rels, metas = [], [], [], []
    for b in range(B):
        h, w = shapes[b]
        f = torch.tensor([w, h, w, h], dtype=torch.float32)
        c, s = rnd(G[b], 2) * 0.6 + 0.2, rnd(G[b], 2) * 0.3 + 0.05
        gb = torch.cat([c - s / 2, c + s / 2], -1) * f
        gl = torch.randint(0, num_classes, (G[b],), generator=g)
        if planted:
            # (distinct labels and distinct (subject, object) pairs: two relations with the same
            # class pair have EQUAL id-cost columns -- r_cls_cost weighs 0 -- and no margin)
            assert G[b] <= num_classes and T[b] <= G[b] * (G[b] - 1)
            gl = torch.randperm(num_classes, generator=g)[:G[b]]
            qs = torch.randperm(KEPT, generator=g)[:G[b]]
            for k, q in enumerate(qs.tolist()):
                bbox[b, q] = torch.cat([c[k], s[k]]) + (rnd(4) - 0.5) * 0.02
                cls[b, q, gl[k]] = 3.0 + rnd(1)
        s_i = torch.randint(0, G[b], (T[b],), generator=g)
        o_i = (s_i + 1 + torch.randint(0, max(G[b] - 1, 1), (T[b],), generator=g)) % G[b]
        pr = torch.randint(1, num_relations + 1, (T[b],), generator=g)
        if planted:
            pairs = torch.randperm(G[b] * (G[b] - 1), generator=g)[:T[b]]
            s_i = pairs // (G[b] - 1)
            o_i = pairs % (G[b] - 1)
            o_i = o_i + (o_i >= s_i).long()
        gt_bboxes.append(gb)
        gt_labels.append(gl)
        gt_rels.append(torch.stack([s_i, o_i, pr], 1))
        metas.append(dict(img_shape=(h, w, 3), batch_input_shape=tuple(batch_shape)))
    sub = torch.randn(B, R, num_classes, generator=g)
    obj = torch.randn(B, R, num_classes, generator=g)
    rel = torch.randn(B, R, num_relations, generator=g)
    if planted:      # one relation query per ground-truth relation with its two classes on top
        for b in range(B):
            rq = torch.randperm(R, generator=g)[:T[b]]
            for k, r in enumerate(rq.tolist()):
                s_k, o_k = gt_rels[b][k, 0], gt_rels[b][k, 1]
                sub[b, r, gt_labels[b][s_k]] += 5.0
                obj[b, r, gt_labels[b][o_k]] += 5.0
    imp = torch.randn(B, KEPT, KEPT, generator=g)
    return dict(cls=cls, bbox=bbox, sub=sub, obj=obj, rel=rel, importance=imp, gt_bboxes=gt_bboxes,
                gt_labels=gt_labels, gt_rels=gt_rels, img_metas=metas, num_classes=num_classes,
                num_relations=num_relations)


# the two cases of the fixture: B = 2 with 3 / 7 boxes and 2 / 9 relations; one image whose
# img_shape lies inside the batch shape
GOLDEN_CASES = dict(a=dict(seed=1, G=(3, 7), T=(2, 9)),
                    b=dict(seed=2, G=(5,), T=(6,), shapes=[(50, 61)]))


def golden_case(name):
    """Fixture case -> (a make_case-shaped dict, the stored reference values)."""
    z = np.load(GOLDEN)
    pre = name + "."
    B = int(z[pre + "B"])
    t = lambda k: torch.from_numpy(z[pre + k])
    case = {k: t(k) for k in ("cls", "bbox", "sub", "obj", "rel", "importance")}
    case.update(gt_bboxes=[t("gt_bboxes.%d" % b) for b in range(B)],
                gt_labels=[t("gt_labels.%d" % b) for b in range(B)],
                gt_rels=[t("gt_rels.%d" % b) for b in range(B)],
                img_metas=[dict(img_shape=tuple(int(v) for v in z[pre + "img_shape.%d" % b]),
                                batch_input_shape=tuple(int(v) for v in z[pre + "batch_shape"]))
                           for b in range(B)],
                num_classes=int(z[pre + "num_classes"]), num_relations=int(z[pre + "num_relations"]))
    ref = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    return case, ref


# -------------------------------------------------------------------------- the reference itself
def load_reference():
    """The reference's CrossHeadBBox class, loaded in place under name-only stubs, with the
    restated assigner / sampler of this module registered in the builders it calls."""
    from oracle import ref_shim
    ref_shim.install_training()
    mod = sys.modules["pairnet.models.relation_heads.pairnet_bbox_head"]
    # (the module bound the inference stub's `multi_apply = None` at import; its builders stay the
    # stubs -- run_reference sets the built assigners, sampler and losses on the instance itself)
    mod.multi_apply = T.multi_apply
    return mod.CrossHeadBBox


def run_reference(case, dtype=torch.float32):
    """`CrossHeadBBox.loss` of the reference on a case, in `dtype` -> (losses, {gradients of their
    sum w.r.t. rel / importance / sub / obj}, per-image AssignResult.gt_inds of both matchers)."""
    Head = load_reference()
    head = Head.__new__(Head)
    torch.nn.Module.__init__(head)
    assigner, sampler, rel_loss, so_loss = build_parts(case["num_classes"], case["num_relations"],
                                                       case.get("cum"))
    seg = sys.modules["pairnet.models.losses.seg_losses"]
    head.__dict__.update(num_classes=case["num_classes"], num_relations=case["num_relations"],
                         num_rel_query=case["rel"].shape[1], bbox_assigner=assigner, sampler=sampler,
                         id_assigner=T.build_assigner(dict(
                             type="IdMatcher", sub_id_cost=dict(type="ClassificationCost", weight=1.0),
                             obj_id_cost=dict(type="ClassificationCost", weight=1.0),
                             r_cls_cost=dict(type="ClassificationCost", weight=0.0))))
    head.rel_cls_loss = rel_loss.to(dtype)
    head.subobj_cls_loss = so_loss
    head.importance_match_loss = seg.BCEWithLogitsLoss(reduction="mean", loss_weight=5.0)
    leaves = {k: case[k].to(dtype).clone().requires_grad_(True)
              for k in ("rel", "importance", "sub", "obj")}
    cls = dict(leaves, cls=case["cls"].to(dtype))
    seen = []
    real_assign, real_id = assigner.assign, head.id_assigner.assign

    def spy(fn):
        def wrapped(*a, **k):
            r = fn(*a, **k)
            seen.append(r.gt_inds.clone())
            return r
        return wrapped
    assigner.assign, head.id_assigner.assign = spy(real_assign), spy(real_id)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)       # (the reference's torch.zeros((100, 100)) target)
    try:
        out = head.loss(cls, dict(bbox=case["bbox"].to(dtype)), case["gt_rels"],
                        [b.to(dtype) for b in case["gt_bboxes"]], case["gt_labels"],
                        case["img_metas"])
        sum(out.values()).backward()
    finally:
        torch.set_default_dtype(old)
    return ({k: v.detach() for k, v in out.items()}, {k: v.grad.detach() for k, v in leaves.items()},
            seen)
