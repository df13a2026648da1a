"""The Mask2Former segmentation losses on device outputs: what trains the masks and the object
classes (`configs/mask2former/baseline_r50_psg.py` cannot be trained without them).

`Mask2FormerLoss.loss(...)` takes what the reference's `MaskFormerHead.loss` takes
(pairnet/models/panoptic_heads/maskformer_head.py:305-312) -- the class and mask logit stacks of
all L decoder layers and the per-image ground truth (labels [G_b]; masks [G_b, hg, wg], 0/1, on one
grid per batch, prepared as for `CrossHead2` by `PSGTr._prepare_gt_masks`; `HalfSizeMasks` is
accepted) -- and returns the same dict
(`loss_cls`, `loss_mask`, `loss_dice`, `d0.loss_cls`, ..., the last layer unprefixed, :340-353) as
0-dim device tensors: the VALUES and, with `grads={}`, the gradient of the SUM of the 3L terms with
respect to the two logit stacks.  `SegmenterHeadGrad` (seg_grad.py) carries those gradients on through
`mask_embed`, `cls_embed`, `post_norm` and the nine masked decoder layers, to the mask feature and the
memory tokens; the FPN side behind the mask feature is not built.

Per layer and image (panoptic_heads/mask2former_head.py:157-221): `num_points` points shared by all
maps, `pn_point_sample_f32` on predictions and ground truth, `pn_mask_match_cost_f32`, then ALL L * B
assignments in ONE `pn_lsa_f32` launch and `pn_seg_targets` for the bookkeeping.  Per layer
(:223-324): `pn_ce_avg_f32` (class weights, avg_factor = class_weight[labels].sum()), the loss points
of every matched mask by `pn_uncertain_points_f32` (panoptic_heads/point_sample.py:32-88),
`pn_point_sample_rows_f32` on predictions and targets, `pn_mask_point_loss_f32` for the sigmoid CE
and the dice term, and `pn_point_scatter_grad_f32` for the mask-logit gradient (csrc/seg_loss.hip).

The random draws are counter-based (`pn_uniform_f32`: Philox4x32-10 at (seed; element / 4, rank,
site, step), site = 4 * layer + {0 assign, 1 candidates, 2 tail}): nothing is uploaded for them and
the same (seed, rank, step) gives the same bits.  `points=` injects the reference's `torch.rand`
draws instead.  Nothing crosses PCIe except the ground truth going up (pinned, non-blocking) and
nothing is waited for: a cost matrix scipy would raise on sets `self.assign_status` (a device
word), leaves that problem's targets at their fills and the other layers unaffected.  A side above
`hip.LSA_MAX_SIDE` (known from shapes) takes scipy on the host, as losses.py does.

`num_total_masks` is this rank's own count, max(M_l, 1); a data-parallel caller passes its
all-reduced mean (the reference's `reduce_mean`, :278) as `num_total_masks=`.  No collective here.
"""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import hip
from .config import ConfigDict
from .losses import _to_dev


class Mask2FormerLoss:
    def __init__(self, num_classes, num_queries, train_cfg=None, loss_cls=None, loss_mask=None,
                 loss_dice=None):
        t = ConfigDict(train_cfg or dict(
            num_points=12544, oversample_ratio=3.0, importance_sample_ratio=0.75,
            mask_assigner=dict(type="MaskHungarianAssigner",
                               cls_cost=dict(type="ClassificationCost", weight=2.0),
                               mask_cost=dict(type="CrossEntropyLossCost", weight=5.0, use_sigmoid=True),
                               dice_cost=dict(type="DiceCost", weight=5.0, pred_act=True, eps=1.0)),
            sampler=dict(type="MaskPseudoSampler")))
        lc = dict(loss_cls or dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=2.0,
                                   reduction="mean", class_weight=[1.0] * num_classes + [0.1]))
        lm = dict(loss_mask or dict(type="CrossEntropyLoss", use_sigmoid=True, reduction="mean",
                                    loss_weight=5.0))
        ld = dict(loss_dice or dict(type="DiceLoss", use_sigmoid=True, activate=True,
                                    reduction="mean", naive_dice=True, eps=1.0, loss_weight=5.0))
        ma = t.get("mask_assigner", t.get("assigner"))
        if ma is None:
            raise NotImplementedError("train_cfg without a mask_assigner")
        want = [(ma["type"], "MaskHungarianAssigner"),
                (ma["cls_cost"]["type"], "ClassificationCost"),
                (ma["mask_cost"]["type"], "CrossEntropyLossCost"), (ma["dice_cost"]["type"], "DiceCost"),
                (t.get("sampler", dict(type="MaskPseudoSampler"))["type"], "MaskPseudoSampler"),
                (lc["type"], "CrossEntropyLoss"), (lm["type"], "CrossEntropyLoss"),
                (ld["type"], "DiceLoss")]
        for got, exp in want:
            if got != exp:
                raise NotImplementedError("%s (built: %s, configs/mask2former/"
                                          "baseline_r50_psg.py:351-389)" % (got, exp))
        if not ma["mask_cost"].get("use_sigmoid", True) or not ma["dice_cost"].get("pred_act", False) \
                or not ma["dice_cost"].get("naive_dice", True) or lc.get("use_sigmoid", False) \
                or lc.get("use_mask", False) or not lm.get("use_sigmoid", False) \
                or not ld.get("use_sigmoid", True) or not ld.get("activate", True) \
                or not ld.get("naive_dice", False) \
                or any(c.get("reduction", "mean") != "mean" for c in (lc, lm, ld)) \
                or any(c.get("class_weight") is not None for c in (lm, ld)) \
                or any(c.get("ignore_index") is not None or c.get("avg_non_ignore", False)
                       for c in (lc, lm)):
            raise NotImplementedError("loss options outside configs/mask2former/"
                                      "baseline_r50_psg.py:351-389")
        self.num_classes, self.Q = int(num_classes), int(num_queries)
        self.num_points = int(t.get("num_points", 12544))
        self.oversample_ratio = float(t.get("oversample_ratio", 3.0))
        self.importance_sample_ratio = float(t.get("importance_sample_ratio", 0.75))
        if self.oversample_ratio < 1 or not 0 <= self.importance_sample_ratio <= 1:
            raise ValueError("oversample_ratio >= 1 and 0 <= importance_sample_ratio <= 1 "
                             "(point_sample.py:57-58)")
        self.c_cls, self.c_mask = float(ma["cls_cost"]["weight"]), float(ma["mask_cost"]["weight"])
        self.c_dice = float(ma["dice_cost"]["weight"])
        self.c_dice_eps = float(ma["dice_cost"].get("eps", 1e-3))
        cw = lc.get("class_weight")
        cw = [1.0] * (num_classes + 1) if cw is None else list(cw)
        if len(cw) != num_classes + 1:
            raise ValueError("loss_cls.class_weight has %d entries for %d class logits"
                             % (len(cw), num_classes + 1))
        self.class_weight = cw
        self.w_cls = float(lc.get("loss_weight", 1.0))
        self.w_mask = float(lm.get("loss_weight", 1.0))
        self.w_dice, self.dice_eps = float(ld.get("loss_weight", 1.0)), float(ld.get("eps", 1e-3))
        self._cw = None
        self.assign_status = None      # device int32 [1] of the last call
        self.last_on_device = False    # whether the last call solved its assignments on the device
        self.last = None               # the last call's targets and points (device tensors)

    # ---- ground truth: one pinned, non-blocking upload of labels + table; masks per image ----
    def _ground_truth(self, gt_labels_list, gt_masks_list, B, h, w, dev):
        from .train_pipeline import HalfSizeMasks
        if len(gt_labels_list) != B or len(gt_masks_list) != B:
            raise ValueError("ground truth for %d images, logits for %d" % (len(gt_labels_list), B))
        labels, masks, hw = [], [], None
        for gl, gm in zip(gt_labels_list, gt_masks_list):
            gl = torch.as_tensor(gl).reshape(-1).to(torch.int64)
            gm = gm.masks if isinstance(gm, HalfSizeMasks) else gm
            gm = gm.to_ndarray() if hasattr(gm, "to_ndarray") else gm
            gm = torch.as_tensor(gm)
            # (the masks keep their own grid -- PSGTr prepares them at half the batch tensor, the
            # logits are at a quarter: point sampling works in normalised coordinates)
            if gm.dim() != 3 or gm.shape[0] != gl.shape[0]:
                raise ValueError("gt_masks: [%d, h, w], got %s" % (gl.shape[0], tuple(gm.shape)))
            if gm.shape[0]:
                hw = hw or tuple(gm.shape[1:])
                if tuple(gm.shape[1:]) != hw or min(hw) <= 0:
                    raise ValueError("gt_masks: one (h, w) for the batch, got %s and %s"
                                     % (hw, tuple(gm.shape[1:])))
                if gm.dtype not in (torch.bool, torch.uint8):
                    gm = (gm != 0)
                gm = _to_dev(gm, dev)
                masks.append(gm.view(torch.uint8) if gm.dtype == torch.bool else gm)
            labels.append(gl)
        G = [int(l.shape[0]) for l in labels]
        gt_all = torch.cat(masks) if masks else torch.zeros((1, h, w), dtype=torch.uint8, device=dev)
        return labels, gt_all.contiguous(), G

    @torch.no_grad()
    @hip.on_device
    def loss(self, all_cls_scores, all_mask_preds, gt_labels_list, gt_masks_list, img_metas,
             grads=None, points=None, seed=0, step=0, num_total_masks=None, rank=0, debug=False):
        """`points`: the reference's draws, to reproduce one of its runs -- either
        dict(assign=[L][B] of [Np, 2], candidates=[L] of [M_l, S, 2], tail=[L] of [M_l, Np - k, 2])
        or dict(assign=..., loss=[L] of [M_l, Np, 2]) (final loss points, selection bypassed);
        every key is optional, a missing one is drawn here.  `grads`: a dict filled with "cls"
        [L, B, Q, C + 1], "mask_rows" int64 [M] (row index into L * B * Q; -1 for a row whose
        assignment failed) and "mask" [M, h, w].  `self.last` keeps the call's targets (labels,
        matched, mcount) and `counts`, the host list n_b = min(Q, G_b) of matched rows per image
        (what `SegmenterHeadGrad.backward` needs to know the rows' images); `debug=True` also keeps its points, keys, candidates, samples and
        coefficients alive there (hundreds of MB at production shapes)."""
        cls = all_cls_scores if torch.is_tensor(all_cls_scores) else torch.stack(list(all_cls_scores))
        mask = all_mask_preds if torch.is_tensor(all_mask_preds) else torch.stack(list(all_mask_preds))
        if cls.dim() != 4 or mask.dim() != 5 or cls.shape[:3] != mask.shape[:3] or \
                cls.dtype != torch.float32 or mask.dtype != torch.float32:
            raise ValueError("cls [L, B, Q, C + 1] and mask [L, B, Q, h, w] fp32 logits, got %s and %s"
                             % (tuple(cls.shape), tuple(mask.shape)))
        cls, mask = cls.contiguous(), mask.contiguous()
        L, B, Q, C1 = cls.shape
        h, w = int(mask.shape[3]), int(mask.shape[4])
        dev = cls.device
        if Q != self.Q or C1 != self.num_classes + 1:
            raise ValueError("logits for %d queries / %d classes, built for %d / %d"
                             % (Q, C1 - 1, self.Q, self.num_classes))
        if B * Q > 4096 or L > 64:
            raise NotImplementedError("B * Q <= 4096 rows and L <= 64 layers per call")
        points = dict(points or {})
        unknown = set(points) - {"assign", "candidates", "tail", "loss"}
        if unknown:
            raise ValueError("points: unknown keys %s" % sorted(unknown))
        labels_h, gt_all, G = self._ground_truth(gt_labels_list, gt_masks_list, B, h, w, dev)
        f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)

        # ---- sizes and the two tables, on the host from shapes alone ----
        n_b = [min(Q, g) for g in G]
        Ml = sum(n_b)
        Mtot = L * Ml
        if Mtot > 65535:
            raise NotImplementedError("at most 65535 matched masks per call")
        g_off = np.concatenate([[0], np.cumsum(G)]).astype(np.int64)
        m_off = np.concatenate([[0], np.cumsum(n_b)]).astype(np.int64)
        lsa_tab, seg_tab, where = [], [], []
        c_off = o_off = 0
        for l in range(L):
            for b in range(B):
                if G[b] == 0:
                    seg_tab += [-1, 0, 0, int(g_off[b]), 0, l * Ml + int(m_off[b])]
                    continue
                seg_tab += [len(where), o_off, n_b[b], int(g_off[b]), G[b], l * Ml + int(m_off[b])]
                lsa_tab += [c_off, Q, G[b], o_off]
                where.append((l, b, c_off, o_off))
                c_off += Q * G[b]
                o_off += n_b[b]
        P = len(where)
        head = torch.tensor(seg_tab + lsa_tab, dtype=torch.int64)
        nh = head.numel()
        if all(not t.is_cuda for t in labels_h):
            buf = torch.empty(nh + int(g_off[-1]), dtype=torch.int64, pin_memory=True)
            torch.cat([head] + labels_h, out=buf)
            up = buf.to(dev, non_blocking=True)
            tabs, gl = up[:nh], up[nh:]
        else:
            tabs, gl = _to_dev(head, dev), torch.cat([_to_dev(t, dev) for t in labels_h])
        if gl.numel() == 0:
            gl = torch.zeros(1, dtype=torch.int64, device=dev)
        seg_tab, lsa_tab = tabs[:6 * L * B].view(L * B, 6), tabs[6 * L * B:].view(P, 4)

        # ---- matching: points, samples and costs of every (layer, image) ----
        Np_draw = self.num_points
        assign = points.get("assign")
        if assign is None and P:
            drawn = f32(L, B * Np_draw * 2)
            hip.uniform(drawn, seed, rank, step, hip.SEG_SITE_ASSIGN, site_stride=4)
            drawn = drawn.view(L, B, Np_draw, 2)
        cost_all = f32(max(c_off, 1))
        assign_pts = {}
        for l, b, co, _ in where:
            if assign is None:
                pts = drawn[l, b]
            else:
                pts = _to_dev(torch.as_tensor(assign[l][b]).reshape(-1, 2), dev).to(torch.float32).contiguous()
            Na = pts.shape[0]
            pred_pts, gt_pts = f32(Q, Na), f32(G[b], Na)
            hip.point_sample(mask[l, b], pts, pred_pts)
            hip.point_sample(gt_all[g_off[b]:g_off[b + 1]], pts, gt_pts)
            hip.mask_match_cost(cls[l, b], gl[g_off[b]:g_off[b + 1]], pred_pts, gt_pts,
                                cost_all[co:co + Q * G[b]].view(Q, G[b]), self.c_cls, self.c_mask,
                                self.c_dice, self.c_dice_eps)
            assign_pts[(l, b)] = pts

        # ---- L * B assignments in one launch (or scipy on the host above the solver's limit) ----
        rows, cols = i32(max(o_off, 1)), i32(max(o_off, 1))
        lsa_status = torch.zeros(max(P, 1), device=dev, dtype=torch.int32)
        self.last_on_device = max([Q] + G) <= hip.LSA_MAX_SIDE
        if P and self.last_on_device:
            hip.lsa(cost_all, lsa_tab, rows, cols, lsa_status, max_cells=Q * max(G))
        elif P:
            host = cost_all.cpu().numpy()
            r_h, c_h = np.zeros(o_off, np.int32), np.zeros(o_off, np.int32)
            for l, b, co, oo in where:
                r, c = linear_sum_assignment(host[co:co + Q * G[b]].reshape(Q, G[b]))
                order = np.argsort(r)
                r_h[oo:oo + n_b[b]], c_h[oo:oo + n_b[b]] = r[order], c[order]
            rows, cols = torch.from_numpy(r_h).to(dev), torch.from_numpy(c_h).to(dev)
        labels = torch.empty(L, B * Q, device=dev, dtype=torch.int64)
        matched = torch.full((Mtot, 4), -1, device=dev, dtype=torch.int64)
        mcount, status = i32(L), i32(1)
        hip.seg_targets(seg_tab, rows, cols, lsa_status, gl, L, B, Q, self.num_classes, labels,
                        matched, mcount, status)
        self.assign_status = status

        # ---- loss_cls ----
        if self._cw is None or self._cw.device != dev:
            self._cw = torch.tensor(self.class_weight, dtype=torch.float32, device=dev)
        out_cls = f32(L)
        cls3 = cls.view(L, B * Q, C1)
        hip.ce_avg(cls3, labels, self._cw, out_cls, self.w_cls)
        if grads is not None:
            g_cls = torch.empty_like(cls)
            hip.ce_avg_grad(cls3, labels, self._cw, g_cls.view(L, B * Q, C1), self.w_cls)

        # ---- loss_mask / loss_dice over the matched masks' loss points ----
        self.last = dict(labels=labels, matched=matched, mcount=mcount, counts=list(n_b))
        if debug:
            self.last.update(assign=assign_pts, rows=rows, cols=cols, lsa_status=lsa_status)
        maps = mask.view(L * B * Q, h, w)
        if Mtot == 0:
            # zero match (mask2former_head.py:285-289): both terms 0, no mask gradient
            out_m = torch.zeros(4 * L, device=dev, dtype=torch.float32)
            idx_pred = torch.empty(0, device=dev, dtype=torch.int64)
            g_mask = f32(0, h, w)
        else:
            ok = matched[:, 0] >= 0
            idx_pred = torch.where(ok, (matched[:, 0] * B + matched[:, 1]) * Q + matched[:, 2],
                                   matched[:, 0])
            idx_gt = matched[:, 3].contiguous()
            cat = lambda seq: torch.cat([_to_dev(torch.as_tensor(t), dev).to(torch.float32)
                                         .reshape(Ml, -1, 2) for t in seq]).contiguous()
            if "loss" in points:
                pts = cat(points["loss"])
                if pts.shape[0] != Mtot:
                    raise ValueError("points['loss']: %d rows for %d matched masks" % (pts.shape[0], Mtot))
                Np = pts.shape[1]
            else:
                Np = self.num_points
                S = int(Np * self.oversample_ratio)
                k = int(self.importance_sample_ratio * Np)
                if "candidates" in points:
                    cand = cat(points["candidates"])
                else:
                    cand = f32(L, Ml * S * 2)
                    hip.uniform(cand, seed, rank, step, hip.SEG_SITE_CANDIDATES, site_stride=4)
                    cand = cand.view(Mtot, S, 2)
                tail = None
                if k < Np and "tail" in points:
                    tail = cat(points["tail"])
                elif k < Np:
                    tail = f32(L, Ml * (Np - k) * 2)
                    hip.uniform(tail, seed, rank, step, hip.SEG_SITE_TAIL, site_stride=4)
                    tail = tail.view(Mtot, Np - k, 2)
                if cand.shape != (Mtot, S, 2) or (tail is not None and tail.shape != (Mtot, Np - k, 2)):
                    raise ValueError("points: candidates [M_l, %d, 2] and tail [M_l, %d, 2] per layer"
                                     % (S, Np - k))
                keys, pts = i32(Mtot, S), f32(Mtot, Np, 2)
                hip.uncertain_points(maps, matched, B, Q, cand, tail, k, keys, pts)
                if debug:
                    self.last.update(keys=keys, candidates=cand, k=k)
            x, t = f32(Mtot, Np), f32(Mtot, Np)
            hip.point_sample_rows(maps, idx_pred, pts, x)
            hip.point_sample_rows(gt_all, idx_gt, pts, t)
            out_m, sums = f32(4 * L), f32(Mtot, 4)
            coef = f32(Mtot, Np) if grads is not None else None
            hip.mask_point_loss(x, t, matched, L, self.w_mask, self.w_dice, self.dice_eps, sums,
                                out_m, coef, 0.0 if num_total_masks is None else float(num_total_masks))
            if debug:
                self.last.update(points=pts, x=x, t=t, sums=sums, coef=coef)
            if grads is not None:
                g_mask = f32(Mtot, h, w)
                scratch = i32(hip.point_scatter_scratch_ints(Mtot, Np, h, w))
                hip.point_scatter_grad(coef, pts, g_mask, scratch)
        if grads is not None:
            grads.update(cls=g_cls, mask_rows=idx_pred, mask=g_mask)
        out = dict(loss_cls=out_cls[L - 1], loss_mask=out_m[L - 1], loss_dice=out_m[2 * L - 1])
        for l in range(L - 1):
            out["d%d.loss_cls" % l] = out_cls[l]
            out["d%d.loss_mask" % l] = out_m[l]
            out["d%d.loss_dice" % l] = out_m[L + l]
        return out
