"""Loss of the plain Deformable-DETR detector on device outputs: [3P] mmdet's
`DeformableDETRHead.loss` / `DETRHead.loss_single` under configs/deformable_detr/od_r101_vg.py:80-94
(the in-tree statement of one term is the commented text at
pairnet/models/relation_heads/pairnet_bbox_head.py:596-642).

One term per decoder layer plus one for the encoder's per-token proposals (matched against the
ground truth with every label set to 0): 3 * (L + 1) values.  Per term

  assignment  HungarianAssigner on FocalLossCost + BBoxL1Cost(xywh) + IoUCost(giou): every problem's
              rows x G cost block in ONE `pn_det_match_cost_f32` launch, then -- where mmdet solves
              them (`linear_sum_assignment(cost.cpu())`) -- scipy on the downloaded blocks; the
              pairs go back as int32.
  loss_cls    FocalLoss (sigmoid) summed over rows * C / max(num_total_pos, 1) (`bg_cls_weight` is
              0 for this head): `pn_det_focal_f32`, all terms in one streaming launch.
  loss_bbox   L1 over the matched rows / the same factor        } `pn_det_box_loss_f32`, one
  loss_iou    1 - GIoU of cxcywh_to_xyxy(.) * factor, both sides } workgroup per term

`num_total_pos = sum_b min(rows, G_b)` is known from shapes, so the factors need no device read.  An
image without ground truth is legal (`filter_empty_gt=False`): all of its rows are background.

`grads={}` receives d(sum of all returned terms) / d of the four forward outputs ("cls", "bbox",
"enc_cls", "enc_bbox"), every element written.  `trace=[]` receives per (term, image) the pairs and
the cost block.

Not built: `device_targets=True` (the encoder term is one SN x G problem per image with SN in the
tens of thousands; `pn_lsa_f32` keeps its state in LDS for sides <= 1024), data-parallel
`reduce_mean` (`group=`), other loss / cost / assigner types.  UNPINNED: the
element value is mmdet's `py_sigmoid_focal_loss`; mmcv's CUDA op differs from it only through its
`log` clamp at |logit| beyond fp32's exponent range.
"""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import hip
from .config import ConfigDict

_WHERE = "configs/deformable_detr/od_r101_vg.py:80-94"


class DeformableDETRLoss:
    def __init__(self, num_classes, loss_cls=None, loss_bbox=None, loss_iou=None, train_cfg=None,
                 sync_cls_avg_factor=True, device_targets=False, group=None):
        if device_targets:
            raise NotImplementedError("device_targets=True: the encoder term's SN x G problems do "
                                      "not fit pn_lsa_f32 (sides <= %d); host mode only"
                                      % hip.LSA_MAX_SIDE)
        if group is not None:
            raise NotImplementedError("group=: one rank only (reduce_mean across ranks is not built)")
        lc = ConfigDict(loss_cls or dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25,
                                         loss_weight=2.0))
        lb = ConfigDict(loss_bbox or dict(type="L1Loss", loss_weight=5.0))
        li = ConfigDict(loss_iou or dict(type="GIoULoss", loss_weight=2.0))
        t = ConfigDict(train_cfg or dict(assigner=dict(
            type="HungarianAssigner", cls_cost=dict(type="FocalLossCost", weight=2.0),
            reg_cost=dict(type="BBoxL1Cost", weight=5.0, box_format="xywh"),
            iou_cost=dict(type="IoUCost", iou_mode="giou", weight=2.0))))
        a = t["assigner"]
        want = [(lc.get("type"), "FocalLoss"), (lb.get("type"), "L1Loss"),
                (li.get("type"), "GIoULoss"), (a.get("type"), "HungarianAssigner"),
                (a["cls_cost"].get("type"), "FocalLossCost"),
                (a["reg_cost"].get("type"), "BBoxL1Cost"), (a["iou_cost"].get("type"), "IoUCost"),
                (t.get("sampler", dict(type="PseudoSampler"))["type"], "PseudoSampler")]
        for got, exp in want:
            if got != exp:
                raise NotImplementedError("%s (built: %s, %s)" % (got, exp, _WHERE))
        if not lc.get("use_sigmoid", False) or lc.get("class_weight") is not None:
            raise NotImplementedError("FocalLoss(use_sigmoid=True) without class weights")
        if a["reg_cost"].get("box_format", "xyxy") != "xywh" \
                or a["iou_cost"].get("iou_mode", "giou") != "giou" \
                or a["cls_cost"].get("binary_input", False):
            raise NotImplementedError("BBoxL1Cost(box_format='xywh'), IoUCost(iou_mode='giou'), "
                                      "FocalLossCost on class logits")
        for c in (lc, lb, li):
            if c.get("reduction", "mean") != "mean":
                raise NotImplementedError("reduction='mean' only")
        self.num_classes = int(num_classes)
        self.alpha, self.gamma = float(lc.get("alpha", 0.25)), float(lc.get("gamma", 2.0))
        self.w_cls = float(lc.get("loss_weight", 1.0))
        self.w_bbox = float(lb.get("loss_weight", 1.0))
        self.w_iou = float(li.get("loss_weight", 1.0))
        self.iou_eps = float(li.get("eps", 1e-6))
        cc = a["cls_cost"]
        self.cost_w = (float(cc.get("weight", 1.0)), float(a["reg_cost"].get("weight", 1.0)),
                       float(a["iou_cost"].get("weight", 1.0)))
        self.cost_focal = dict(alpha=float(cc.get("alpha", 0.25)), gamma=float(cc.get("gamma", 2.0)),
                               eps=float(cc.get("eps", 1e-12)))
        self.sync_cls_avg_factor = bool(sync_cls_avg_factor)     # (one rank: the mean is itself)
        self._terms = {}

    def _term_ids(self, L, B, Q, SN, dev):
        """Per-row term id of the concatenated rows: input-independent, kept per shape."""
        key = (L, B, Q, SN, str(dev))
        t = self._terms.get(key)
        if t is None:
            if len(self._terms) >= 8:
                self._terms.clear()
            host = torch.cat([torch.arange(L, dtype=torch.int32).repeat_interleave(B * Q),
                              torch.full((B * SN,), L, dtype=torch.int32)])
            t = self._terms[key] = host.to(dev)
        return t

    @staticmethod
    def keys(L):
        """mmdet's key order: the last layer, the encoder's proposals, then d0 .. d{L-2}."""
        out = ["loss_cls", "loss_bbox", "loss_iou", "enc_loss_cls", "enc_loss_bbox", "enc_loss_iou"]
        for i in range(L - 1):
            out += ["d%d.loss_cls" % i, "d%d.loss_bbox" % i, "d%d.loss_iou" % i]
        return out

    @torch.no_grad()
    def loss(self, all_cls_scores, all_bbox_preds, enc_cls_scores, enc_bbox_preds, gt_bboxes_list,
             gt_labels_list, img_metas, gt_bboxes_ignore=None, grads=None, trace=None,
             device_targets=False, group=None):
        """mmdet's signature -> its 3 * (L + 1) keys as 0-dim device tensors (module docstring)."""
        assert gt_bboxes_ignore is None, "Only supports for gt_bboxes_ignore setting to None."
        if device_targets:
            raise NotImplementedError("device_targets=True is not built (module docstring)")
        if group is not None:
            raise NotImplementedError("group=: one rank only")
        L, B, Q, C = all_cls_scores.shape
        dev = all_cls_scores.device
        if enc_cls_scores is None or enc_bbox_preds is None:
            raise NotImplementedError("the two-stage form: enc_cls_scores / enc_bbox_preds")
        SN = enc_cls_scores.shape[1]
        if C != self.num_classes or tuple(all_bbox_preds.shape) != (L, B, Q, 4) \
                or tuple(enc_cls_scores.shape) != (B, SN, C) \
                or tuple(enc_bbox_preds.shape) != (B, SN, 4):
            raise ValueError("outputs: [L, B, Q, %d], [L, B, Q, 4], [B, SN, %d], [B, SN, 4]"
                             % (self.num_classes, self.num_classes))
        if not (len(img_metas) == len(gt_bboxes_list) == len(gt_labels_list) == B):
            raise ValueError("img_metas / gt_bboxes / gt_labels for a batch of %d" % B)
        T = L + 1
        if max(Q, SN) > hip.DET_MAX_ROWS:
            raise NotImplementedError("at most %d rows per term and image" % hip.DET_MAX_ROWS)
        if T > hip.DET_MAX_TERMS:
            raise NotImplementedError("at most %d decoder layers" % (hip.DET_MAX_TERMS - 1))
        with torch.cuda.device(dev):
            return self._loss(all_cls_scores, all_bbox_preds, enc_cls_scores, enc_bbox_preds,
                              gt_bboxes_list, gt_labels_list, img_metas, grads, trace,
                              (L, B, Q, C, SN, T), dev)

    def _loss(self, all_cls, all_box, enc_cls, enc_box, gt_bboxes_list, gt_labels_list, img_metas,
              grads, trace, dims, dev):
        L, B, Q, C, SN, T = dims
        n_dec = L * B * Q
        rows = n_dec + B * SN
        # ---- the rows of all terms, concatenated: decoder layers, then the proposals ----
        X = torch.cat([all_cls.reshape(n_dec, C), enc_cls.reshape(B * SN, C)])
        PB = torch.cat([all_box.reshape(n_dec, 4), enc_box.reshape(B * SN, 4)])
        # ---- ground truth and the problem table: host work from shapes ----
        gbs, gls, Gs = [], [], []
        for i in range(B):
            gb = torch.as_tensor(gt_bboxes_list[i]).detach().cpu().reshape(-1, 4).to(torch.float32)
            gl = torch.as_tensor(gt_labels_list[i]).detach().cpu().reshape(-1).to(torch.int64)
            if gb.shape[0] != gl.shape[0]:
                raise ValueError("image %d: %d labels for %d boxes" % (i, gl.shape[0], gb.shape[0]))
            if gb.shape[0] > hip.DET_MAX_G:
                raise NotImplementedError("at most %d boxes per image" % hip.DET_MAX_G)
            gbs.append(gb)
            gls.append(gl)
            Gs.append(int(gb.shape[0]))
        NG = sum(Gs)
        g_off = [sum(Gs[:i]) for i in range(B)]
        factor = torch.tensor([[m["img_shape"][1], m["img_shape"][0]] * 2 for m in img_metas],
                              dtype=torch.float32)
        probs, tab, c_off = [], [], 0          # (term, image, rows, row offset, cost offset)
        for t in range(T):
            n = Q if t < L else SN
            for b in range(B):
                if Gs[b] == 0:
                    continue
                roff = (t * B + b) * Q if t < L else n_dec + b * SN
                probs.append((t, b, n, roff, c_off))
                # (labels: the image's own for a decoder layer, the zeros behind them for the
                # proposals' binarised labels)
                tab += [c_off, n, Gs[b], g_off[b] + (NG if t == L else 0), g_off[b], roff]
                c_off += n * Gs[b]
        avg = [float(max(sum(min(Q if t < L else SN, g) for g in Gs), 1)) for t in range(T)]
        avg_dev = torch.tensor(avg, dtype=torch.float32).to(dev, non_blocking=True)
        fac_dev = factor.to(dev, non_blocking=True)
        pairs_host, term_off = [], [0]
        gt_dev = None
        if probs:
            gt_dev = torch.cat(gbs).to(dev, non_blocking=True)
            lab_dev = torch.cat(gls + [torch.zeros(NG, dtype=torch.int64)]).to(dev, non_blocking=True)
            tab_dev = torch.tensor(tab, dtype=torch.int64).view(-1, 6).to(dev, non_blocking=True)
            pfac = fac_dev[torch.tensor([p[1] for p in probs]).to(dev)].contiguous()
            cost_all = torch.empty(c_off, device=dev, dtype=torch.float32)
            hip.det_match_cost(X, PB, lab_dev, gt_dev, pfac, tab_dev, cost_all,
                               max(p[2] * Gs[p[1]] for p in probs), *self.cost_w, **self.cost_focal)
            cost_host = cost_all.cpu().numpy()          # (host, as mmdet: the one wait of the call)
            k = 0
            for t in range(T):
                while k < len(probs) and probs[k][0] == t:
                    _, b, n, roff, co = probs[k]
                    cost = cost_host[co:co + n * Gs[b]].reshape(n, Gs[b])
                    r, c = linear_sum_assignment(cost)
                    order = np.argsort(r, kind="stable")     # PseudoSampler: ascending row order
                    r, c = r[order], c[order]
                    if trace is not None:
                        trace.append(dict(term=t, image=b, rows=r.astype(np.int64),
                                          cols=c.astype(np.int64),
                                          cost=torch.from_numpy(cost.copy())))
                    pairs_host.append(np.stack([r + roff, c + g_off[b], np.full_like(r, b),
                                                np.full_like(r, t)], 1))
                    k += 1
                term_off.append(sum(p.shape[0] for p in pairs_host))
        else:
            term_off += [0] * T
        M = term_off[-1]
        # ---- per-row labels: background, then a scatter over the pairs (rows are unique) ----
        labels = torch.full((rows,), C, device=dev, dtype=torch.int32)
        toff_dev = torch.tensor(term_off, dtype=torch.int32).to(dev, non_blocking=True)
        pairs_dev = None
        if M:
            ph = np.concatenate(pairs_host).astype(np.int32)
            gl_all = torch.cat(gls).numpy()
            vals = np.where(ph[:, 3] == L, 0, gl_all[ph[:, 1]]).astype(np.int32)
            up = torch.from_numpy(np.concatenate([ph.reshape(-1), vals])).to(dev, non_blocking=True)
            pairs_dev = up[:4 * M].view(M, 4)
            labels[pairs_dev[:, 0].long()] = up[4 * M:]
        # ---- the three kernels ----
        gX = torch.empty(rows, C, device=dev, dtype=torch.float32)
        gB = torch.zeros(rows, 4, device=dev, dtype=torch.float32)
        partial = torch.empty(hip.det_focal_partials(rows, C, T), device=dev, dtype=torch.float32)
        out_c = torch.empty(T, device=dev, dtype=torch.float32)
        out_b = torch.empty(T, 2, device=dev, dtype=torch.float32)
        hip.det_focal(X, labels, self._term_ids(L, B, Q, SN, dev), avg_dev, gX, partial, out_c,
                      self.w_cls, self.alpha, self.gamma)
        hip.det_box_loss(PB, gt_dev, fac_dev, pairs_dev, toff_dev, avg_dev, gB, out_b, self.w_bbox,
                         self.w_iou, self.iou_eps)
        if grads is not None:
            grads["cls"], grads["enc_cls"] = gX[:n_dec].view(L, B, Q, C), gX[n_dec:].view(B, SN, C)
            grads["bbox"], grads["enc_bbox"] = gB[:n_dec].view(L, B, Q, 4), gB[n_dec:].view(B, SN, 4)
        out = {}
        for t in range(T):
            pre = "" if t == L - 1 else ("enc_" if t == L else "d%d." % t)
            out[pre + "loss_cls"] = out_c[t]
            out[pre + "loss_bbox"], out[pre + "loss_iou"] = out_b[t, 0], out_b[t, 1]
        return {k: out[k] for k in self.keys(L)}
