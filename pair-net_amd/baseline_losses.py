"""The relation terms of the sibling head's loss on device outputs: `r_loss_cls`,
`loss_subject_match` and `loss_object_match` of the reference's `CrossHeadBaseline.loss`
(pairnet/models/relation_heads/baseline.py:655-694, 828-907), reported for the last decoder layer
(:523-526) -- what `configs/mask2former/baseline_r50_psg.py` adds to the 27 Mask2Former terms of
seg_losses.py.

`BaselineRelationLoss.loss(...)` takes the three logit blocks the head returns (`rel` [B, R, Cr + 1],
`subject_scores` / `object_scores` [B, R, Q]), the per-image ground-truth relations [Gr_b, 3] (subject
object, object object, predicate) and the segmentation matching of the same call
(`Mask2FormerLoss.last["matched"]`; the rows of the last layer are read) and returns the three terms
as 0-dim device tensors: the VALUES and, with `grads={}`, the gradient of their SUM with respect to
the three blocks.  Carrying those gradients on into `rel_cls_embed`, the query-update MLPs and the
decoders is not built.

Per call (csrc/rel_loss.hip): `pn_rel_id_cost_f32` fills every image's [R, Gr_b] cost block
(OldIdMatcher, approaches/matcher.py:279-351: -softmax three times, on the matched query of each
related object), ONE `pn_lsa_f32` launch solves the B assignments, `pn_rel_targets` writes the labels
and the positive rows' id targets, `pn_id_ce_f32` the two MultilabelCrossEntropy terms
(losses/seg_losses.py:47-57: log-softmax over the image's matched queries only) and their gradients,
`pn_ce_avg_f32` / `pn_ce_avg_grad_f32` the class term.  The number of launches does not depend on B.
Nothing crosses PCIe except the relations and the table going up (pinned, non-blocking) and nothing
is waited for: what the reference would raise on sets `self.assign_status` (a device word, bits in
include/pairnet_hip.h) and leaves that image's labels at 0 and its id rows out.  A side above
`hip.LSA_MAX_SIDE` (known from shapes) takes scipy on the host, as seg_losses.py does.
"""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import hip
from .config import ConfigDict
from .losses import _to_dev


class BaselineRelationLoss:
    def __init__(self, num_relations, num_obj_query, num_rel_query, train_cfg=None,
                 rel_loss_cls=None, sub_id_loss=None, obj_id_loss=None):
        t = ConfigDict(train_cfg or dict(id_assigner=dict(
            type="OldIdMatcher", sub_id_cost=dict(type="ClassificationCost", weight=1.0),
            obj_id_cost=dict(type="ClassificationCost", weight=1.0),
            r_cls_cost=dict(type="ClassificationCost", weight=1.0))))
        ia = t.get("id_assigner")
        if ia is None:
            raise NotImplementedError("train_cfg without an id_assigner")
        rc = dict(rel_loss_cls or dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=2.0,
                                       reduction="mean",
                                       class_weight=[0.02] + [1.0] * num_relations))
        sl = dict(sub_id_loss or dict(type="MultilabelCrossEntropy", loss_weight=2.0))
        ol = dict(obj_id_loss or dict(type="MultilabelCrossEntropy", loss_weight=2.0))
        costs = [dict(ia.get(k) or dict(type="ClassificationCost", weight=1.0))
                 for k in ("sub_id_cost", "obj_id_cost", "r_cls_cost")]
        want = [(ia["type"], "OldIdMatcher")] + [(c["type"], "ClassificationCost") for c in costs] + \
            [(rc["type"], "CrossEntropyLoss"), (sl["type"], "MultilabelCrossEntropy"),
             (ol["type"], "MultilabelCrossEntropy")]
        for got, exp in want:
            if got != exp:
                raise NotImplementedError("%s (built: %s, configs/mask2former/"
                                          "baseline_r50_psg.py:336-350, 373-378)" % (got, exp))
        if rc.get("use_sigmoid", False) or rc.get("use_mask", False) \
                or rc.get("reduction", "mean") != "mean" or rc.get("ignore_index") is not None \
                or rc.get("avg_non_ignore", False) \
                or any(c.get("reduction", "mean") != "mean" for c in (sl, ol)):
            raise NotImplementedError("loss options outside configs/mask2former/"
                                      "baseline_r50_psg.py:336-350")
        self.num_relations = int(num_relations)
        self.Q, self.R = int(num_obj_query), int(num_rel_query)
        if max(self.Q, self.R) > hip.REL_MAX_SIDE:
            raise NotImplementedError("at most %d object / relation queries" % hip.REL_MAX_SIDE)
        self.c_sub, self.c_obj, self.c_rel = (float(c.get("weight", 1.0)) for c in costs)
        cw = rc.get("class_weight")
        if cw is None or isinstance(cw, (int, float)):
            cw = [1.0 if cw is None else float(cw)] * (num_relations + 1)
        if len(cw) != num_relations + 1:
            raise ValueError("rel_loss_cls.class_weight has %d entries for %d relation logits"
                             % (len(cw), num_relations + 1))
        self.class_weight = list(cw)
        self.w_rel = float(rc.get("loss_weight", 1.0))
        self.w_sub, self.w_obj = float(sl.get("loss_weight", 1.0)), float(ol.get("loss_weight", 1.0))
        self._cw = None
        self.assign_status = None      # device int32 [1] of the last call
        self.last_on_device = False    # whether the last call solved its assignments on the device
        self.last = None               # the last call's targets (device tensors)

    @torch.no_grad()
    @hip.on_device
    def loss(self, rel, subject_scores, object_scores, gt_rels_list, matched, B, grads=None,
             num_gts=None):
        """`matched`: int64 [L * sum_b min(Q, G_b), 4] as `Mask2FormerLoss.last["matched"]` holds it
        (layer, image, query, ground-truth object counted over the batch), the last layer's rows are
        used; `num_gts`: the G_b (host ints; the layout of `matched` follows from them).  `grads`: a
        dict filled with "rel" [B, R, Cr + 1], "subject_scores" and "object_scores" [B, R, Q].
        `self.last` keeps r_labels [B * R], pos [P, 4] (image, row, subject column, object column),
        the cost blocks, the assignment and the uploaded table."""
        R, Q, C1 = self.R, self.Q, self.num_relations + 1
        B = int(B)
        for name, t, last in (("rel", rel, C1), ("subject_scores", subject_scores, Q),
                              ("object_scores", object_scores, Q)):
            if not torch.is_tensor(t) or tuple(t.shape) != (B, R, last) or t.dtype != torch.float32:
                raise ValueError("%s: fp32 [%d, %d, %d], got %s" % (
                    name, B, R, last, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        if B * R > 4096:
            raise NotImplementedError("B * R <= 4096 rows per call")
        if num_gts is None or len(num_gts) != B or len(gt_rels_list) != B:
            raise ValueError("num_gts and gt_rels_list: one entry per image (%d)" % B)
        G = [int(g) for g in num_gts]
        rels = []
        for b, gr in enumerate(gt_rels_list):
            gr = torch.as_tensor(gr)
            if gr.numel() == 0:
                # (the reference fails at torch.stack([]), baseline.py:846; the dataset drops such images)
                raise ValueError("image %d has no ground-truth relation" % b)
            if gr.dim() != 2 or gr.shape[1] != 3:
                raise ValueError("gt_rels: [Gr, 3], got %s" % (tuple(gr.shape),))
            if G[b] > Q:
                raise ValueError("image %d: %d ground-truth objects for %d queries (the reference's own "
                                 "indexing fails, baseline.py:829-830)" % (b, G[b], Q))
            gr = gr.to(torch.int64)
            if not gr.is_cuda:      # (a device tensor is range-checked on the device: status bit 4)
                if int(gr[:, :2].min()) < 0 or int(gr[:, :2].max()) >= G[b]:
                    raise ValueError("image %d: gt_rels objects outside [0, %d)" % (b, G[b]))
                if int(gr[:, 2].min()) < 1 or int(gr[:, 2].max()) > self.num_relations:
                    raise ValueError("image %d: gt_rels predicates outside [1, %d]"
                                     % (b, self.num_relations))
            rels.append(gr)
        dev = rel.device
        Gr = [int(g.shape[0]) for g in rels]
        n_b = [min(Q, g) for g in G]
        Ml = sum(n_b)
        if not torch.is_tensor(matched) or matched.dim() != 2 or matched.shape[1] != 4 or \
                matched.dtype != torch.int64 or matched.shape[0] == 0 or matched.shape[0] % Ml:
            raise ValueError("matched: int64 [L * %d, 4]" % Ml)
        matched = _to_dev(matched, dev).contiguous()
        base = matched.shape[0] - Ml                 # the last layer's rows
        P_b = [min(R, g) for g in Gr]
        tab, lsa_tab = [], []
        c_off = r_off = m_off = g_off = p_off = 0
        for b in range(B):
            tab += [c_off, Gr[b], r_off, base + m_off, n_b[b], g_off, G[b], p_off]
            lsa_tab += [c_off, R, Gr[b], p_off]
            c_off, r_off, m_off = c_off + R * Gr[b], r_off + Gr[b], m_off + n_b[b]
            g_off, p_off = g_off + G[b], p_off + P_b[b]
        head = torch.tensor(tab + lsa_tab, dtype=torch.int64)
        nh = head.numel()
        if all(not t.is_cuda for t in rels):
            buf = torch.empty(nh + 3 * r_off, dtype=torch.int64, pin_memory=True)
            torch.cat([head] + [t.reshape(-1) for t in rels], out=buf)
            up = buf.to(dev, non_blocking=True)
            tabs, gt_rels = up[:nh], up[nh:].view(r_off, 3)
        else:
            tabs = _to_dev(head, dev)
            gt_rels = torch.cat([_to_dev(t, dev) for t in rels]).contiguous()
        tab, lsa_tab = tabs[:8 * B].view(B, 8), tabs[8 * B:].view(B, 4)
        f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
        rel, sub, obj = rel.contiguous(), subject_scores.contiguous(), object_scores.contiguous()

        # ---- cost blocks, B assignments, targets ----
        cost = f32(c_off)
        hip.rel_id_cost(rel, sub, obj, gt_rels, matched, tab, cost, self.c_sub, self.c_obj, self.c_rel)
        rows, cols = i32(p_off), i32(p_off)
        lsa_status = torch.zeros(B, device=dev, dtype=torch.int32)
        self.last_on_device = max([R] + Gr) <= hip.LSA_MAX_SIDE
        if self.last_on_device:
            hip.lsa(cost, lsa_tab, rows, cols, lsa_status, max_cells=R * max(Gr))
        else:
            host = cost.cpu().numpy()
            r_h, c_h = np.zeros(p_off, np.int32), np.zeros(p_off, np.int32)
            co = po = 0
            for b in range(B):
                r, c = linear_sum_assignment(host[co:co + R * Gr[b]].reshape(R, Gr[b]))
                order = np.argsort(r)
                r_h[po:po + P_b[b]], c_h[po:po + P_b[b]] = r[order], c[order]
                co, po = co + R * Gr[b], po + P_b[b]
            rows, cols = torch.from_numpy(r_h).to(dev), torch.from_numpy(c_h).to(dev)
        r_labels = torch.empty(B * R, device=dev, dtype=torch.int64)
        pos, status = i32(p_off, 4), i32(1)
        hip.rel_targets(tab, rows, cols, lsa_status, gt_rels, matched, R, Q, C1, r_labels, pos, status)
        self.assign_status = status

        # ---- the two id terms and r_loss_cls ----
        out_id, row_loss, out_cls = f32(2), f32(p_off, 2), f32(1)
        g_sub = torch.empty_like(sub) if grads is not None else None
        g_obj = torch.empty_like(obj) if grads is not None else None
        hip.id_ce(sub, obj, matched, tab, pos, self.w_sub, self.w_obj, row_loss, out_id, g_sub, g_obj)
        if self._cw is None or self._cw.device != dev:
            self._cw = torch.tensor(self.class_weight, dtype=torch.float32, device=dev)
        rel3, lab2 = rel.view(1, B * R, C1), r_labels.view(1, B * R)
        hip.ce_avg(rel3, lab2, self._cw, out_cls, self.w_rel)
        if grads is not None:
            g_rel = torch.empty_like(rel)
            hip.ce_avg_grad(rel3, lab2, self._cw, g_rel.view(1, B * R, C1), self.w_rel)
            grads.update(rel=g_rel, subject_scores=g_sub, object_scores=g_obj)
        self.last = dict(r_labels=r_labels, pos=pos, cost=cost, rows=rows, cols=cols,
                         lsa_status=lsa_status, row_loss=row_loss, tab=tab, gt_rels=gt_rels,
                         matched=matched)
        return dict(r_loss_cls=out_cls[0], loss_subject_match=out_id[0], loss_object_match=out_id[1])
