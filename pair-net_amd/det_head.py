"""DeformableDETRHead on MI355X: the plain detector the box head's trunk is initialised from
(configs/deformable_detr/od_r101_vg.py:26-85, od_rnext101_vg.py; [3P] mmdet `DeformableDETRHead`,
two-stage and box-refining).

The trunk -- encoder, per-token proposals, six box-refining decoder layers -- is `CrossHeadBBox`'s
(bbox_head.py), by inheritance: this class drops the relation stage (its parameters, buffers and
stage B half) and adds what the detector's own surface needs: every decoder layer's class logits
(`cls_branches[i]` inside the decoder loop), the four outputs of mmdet's `forward`, box results
(`get_bboxes` / `simple_test`: mmdet `DETRHead._get_bboxes_single`) and the detection loss
(det_losses.py).  `num_query` is the trunk's proposal count.

State-dict names are mmdet's, restated from memory (UNPINNED): `transformer.*`,
`cls_branches.0-6.*`, `reg_branches.0-6.{0,2,4}.*`; the two-stage form has no `query_embedding`.

Eval mode only: the trunk's dropout sites are not drawn.  Not built: the one-stage form and the form
without box refinement.

Scheduling: stage A (encoder, proposals) replays as a hipGraph under `use_graphs` like the base
class's; stage B (the decoder loop) always runs eagerly here -- the loop has two forms (all layers'
logits, or the last layer's only) that share one plan, and no graph of either is captured.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import hip
from .bbox_head import CrossHeadBBox
from .config import ConfigDict


class DeformableDETRHead(CrossHeadBBox):
    """Drop-in for mmdet's `DeformableDETRHead(as_two_stage=True, with_box_refine=True)`."""

    def __init__(self, num_classes, in_channels=2048, num_query=100, num_reg_fcs=2,
                 transformer=None, sync_cls_avg_factor=False, as_two_stage=False,
                 with_box_refine=False,
                 positional_encoding=dict(type="SinePositionalEncoding", num_feats=128,
                                          normalize=True),
                 loss_cls=None, loss_bbox=None, loss_iou=None, train_cfg=None,
                 test_cfg=dict(max_per_img=100), init_cfg=None, embed_dims=256, **kwargs):
        if kwargs:
            raise TypeError("DeformableDETRHead: unexpected keywords %s" % sorted(kwargs))
        if transformer is None:
            raise ValueError("DeformableDETRHead needs `transformer=`")
        transformer = ConfigDict(transformer)
        if not (as_two_stage and with_box_refine):
            raise NotImplementedError("two-stage, box-refining form only (as_two_stage=True, "
                                      "with_box_refine=True; see the module docstring)")
        self._read_trunk_cfg(transformer, positional_encoding, embed_dims, num_reg_fcs)
        loss_cls = loss_cls or dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25,
                                    loss_weight=2.0)
        if not loss_cls.get("use_sigmoid", False):
            raise NotImplementedError("a sigmoid classifier (FocalLoss, use_sigmoid=True)")
        self.num_classes = self.cls_out_channels = num_classes
        self.num_query = self.num_queries = self.num_proposals = int(num_query)
        self.KEPT = self.num_proposals          # (no query selection behind the decoder)
        self.use_mask = False
        self.test_cfg, self.train_cfg = ConfigDict(test_cfg or dict(max_per_img=100)), train_cfg
        self.sync_cls_avg_factor = sync_cls_avg_factor
        self._loss_cfg = dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_iou=loss_iou,
                              train_cfg=train_cfg, sync_cls_avg_factor=sync_cls_avg_factor)
        self._loss = None
        if self.num_levels != 4 or not 1 <= self.num_proposals <= 512 or num_classes > 256 \
                or self.num_dec_layers + 1 > hip.DET_MAX_TERMS:
            raise NotImplementedError("4 levels, <= 512 queries, <= 256 classes")
        self.all_layers = True          # forward(): every layer's logits; the results path: last
        self._init_trunk_state()

    # ------------------------------------------------------------------ params
    def param_shapes(self):
        """mmdet's names (UNPINNED): the trunk's and the L + 1 class / box branches -- the subset
        of `CrossHeadBBox.param_shapes()` with these prefixes, in its order."""
        s = OrderedDict()
        self._trunk_param_shapes(s)
        self._branch_param_shapes(s)
        return s

    def _pack(self):
        if self.device is None or self.device.type != "cuda":
            raise RuntimeError("DeformableDETRHead runs on an MI355X only: call .to('cuda:0'); "
                               "there is no CPU path")
        hip.lib()
        w = {k: v.to(self.device).contiguous() for k, v in self._params.items()}
        self._pack_trunk(w)
        self.w = w

    # ------------------------------------------------------------------ buffers
    def _layout(self, pl, E, B, shapes, own_tokens):
        self._layout_trunk(pl, E, B, shapes, own_tokens)
        pl.scr = E(hip.attn_scratch_floats(B, self.num_proposals, self.num_proposals))

    # the references of all layers and the logits of all layers as one tensor each: what forward()
    # returns are views of them
    def _layout_refs(self, pl, E, BP):
        pl.ref_all = E(self.num_dec_layers + 1, BP, 4)
        return [pl.ref_all[i] for i in range(self.num_dec_layers + 1)]

    def _layout_classes(self, pl, E, B, P, nc):
        pl.all_cls = E(self.num_dec_layers, B, P, nc)
        return pl.all_cls[self.num_dec_layers - 1]

    def _layout_kept(self, pl, E, B, P, K, nc):
        pass                            # (no query selection: nothing is ranked or gathered)

    # ------------------------------------------------------------------- stages
    def _layer_outputs(self, i, pl):
        """Layer i's class logits (mmdet: `cls_branches[lvl](hs[lvl])`); the last layer's are the
        trunk's own `pl.classes`."""
        nl = self.num_dec_layers
        if self.all_layers and i < nl - 1:
            w = self.w
            hip.linear(pl.x, w["cls_branches.%d.weight" % i], w["cls_branches.%d.bias" % i],
                       pl.all_cls[i].view(pl.B * self.num_proposals, -1))

    def _stage_b(self, pl):
        self._decoder(pl)

    def _run_stage_on(self, which, pl, feats, cur):
        if which == "b":                 # (both forms of the decoder loop share the plan)
            self._stage_b(pl)
            return
        super()._run_stage_on(which, pl, feats, cur)

    def _outputs(self, pl):
        L, B, P = self.num_dec_layers, pl.B, self.num_proposals
        return (pl.all_cls, pl.ref_all[1:].view(L, B, P, 4), pl.enc_cls, pl.enc_box)

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    @hip.on_device
    def forward(self, mlvl_feats, img_metas, slot=0, all_layers=True):
        """mmdet's four outputs as device tensors: all_cls_scores [L, B, Q, C], all_bbox_preds
        [L, B, Q, 4] (normalised cxcywh, post-sigmoid), enc_cls_scores [B, SN, C], enc_bbox_preds
        [B, SN, 4] (post-sigmoid; invalid tokens carry sigmoid(+inf) = 1).  Views of per-shape
        buffers that the next forward() of the same shape overwrites.  `all_layers=False` (the
        inference path) computes the last layer's logits only: all_cls_scores[:-1] is then stale."""
        B, shapes, _ = self._check_feats(mlvl_feats, img_metas)
        pl = self._plan(B, shapes, None, slot)
        self.all_layers = bool(all_layers)
        try:
            self._run_stage("a", pl, mlvl_feats)
            self._run_stage("b", pl)
        finally:
            self.all_layers = True
        self._last_plan = pl
        return self._outputs(pl)

    __call__ = forward

    def forward_train(self, *a, **kw):
        raise NotImplementedError(
            "forward_train + autograd is not how this head trains: `val_det_losses()` / `loss()` "
            "give mmdet's loss values and `loss(..., grads={})` their gradients w.r.t. the four "
            "forward outputs (INTEGRATION.md); the backward behind them is not built")

    # --------------------------------------------------------------------- loss
    def loss_object(self):
        if self._loss is None:
            from .det_losses import DeformableDETRLoss
            self._loss = DeformableDETRLoss(self.num_classes, **self._loss_cfg)
        return self._loss

    def loss(self, all_cls_scores, all_bbox_preds, enc_cls_scores, enc_bbox_preds, gt_bboxes_list,
             gt_labels_list, img_metas, gt_bboxes_ignore=None, **kw):
        """mmdet's `DeformableDETRHead.loss`: the 3 * (L + 1) keys as 0-dim device tensors
        (det_losses.py; `grads={}`, `trace=[]`)."""
        return self.loss_object().loss(all_cls_scores, all_bbox_preds, enc_cls_scores,
                                       enc_bbox_preds, gt_bboxes_list, gt_labels_list, img_metas,
                                       gt_bboxes_ignore=gt_bboxes_ignore, **kw)

    def val_losses(self, *a, **kw):
        raise NotImplementedError("DeformableDETRHead: use val_det_losses(x, img_metas, gt_bboxes, "
                                  "gt_labels)")

    def val_det_losses(self, x, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None, **kw):
        """The values of mmdet's `forward_train`: `outs = self(x, img_metas)`, then
        `loss(*outs, gt_bboxes, gt_labels, img_metas)`.  Forward only."""
        outs = self.forward(x, img_metas)
        return self.loss(*outs, gt_bboxes, gt_labels, img_metas,
                         gt_bboxes_ignore=gt_bboxes_ignore, **kw)

    # ---------------------------------------------------------- post-processing
    @torch.no_grad()
    @hip.on_device
    def get_bboxes(self, all_cls_scores, all_bbox_preds, enc_cls_scores=None, enc_bbox_preds=None,
                   img_metas=None, rescale=False):
        """mmdet `DETRHead.get_bboxes` / `_get_bboxes_single` for a sigmoid classifier, the whole
        batch in two launches: the best `max_per_img` of each image's Q * C last-layer scores, label
        = index mod C, query = index div C, cxcywh -> xyxy * img_shape, clamped to the image,
        divided by `scale_factor` when `rescale`.  Returns (det [B, K, 5], labels [B, K]) on the
        device.

        The ranking is `pn_topk_strided_f32` on the LOGITS: the sigmoid is monotone, so the order is
        mmdet's wherever it is defined.  Where two sigmoid values round together torch's own order
        is unspecified; here ties go to the smaller flat index."""
        cls, box = all_cls_scores[-1].contiguous(), all_bbox_preds[-1].contiguous()
        B, Q, C = cls.shape
        K = min(int(self.test_cfg.get("max_per_img", self.num_query)), Q * C)
        if K > 512 or Q * C > 65536:
            raise NotImplementedError("max_per_img <= 512, Q * C <= 65536")
        dev = cls.device
        i64 = lambda: torch.empty(B, K, device=dev, dtype=torch.int64)
        idx, qt, rm, labels = i64(), i64(), i64(), i64()
        det = torch.empty(B, K, 5, device=dev, dtype=torch.float32)
        meta = []
        for m in img_metas:
            sf = m.get("scale_factor", 1.0)
            sf = [float(v) for v in sf] if hasattr(sf, "__len__") else [float(sf)] * 4
            meta.append([float(m["img_shape"][0]), float(m["img_shape"][1])] + sf)
        meta = torch.tensor(meta, dtype=torch.float32).to(dev, non_blocking=True)
        hip.topk_strided(cls, 1, Q * C, idx, qt, rm, B, Q * C, C, K)
        hip.det_results(cls, box, idx, meta, det, labels, rescale)
        return det, labels

    @staticmethod
    def bbox2result(det, labels, num_classes):
        """mmdet's `bbox2result` of one image on the downloaded K rows: `num_classes` arrays
        [n_c, 5] in rank order."""
        det, labels = np.asarray(det, dtype=np.float32), np.asarray(labels)
        return [det[labels == c] for c in range(num_classes)]

    def simple_test(self, feats, img_metas, rescale=False):
        """`simple_test_bboxes` + `bbox2result`: one list per image of `num_classes` arrays
        [n_c, 5] (x1, y1, x2, y2, score).  Grouping by class is host work on the K rows."""
        outs = self.forward(feats, img_metas, all_layers=False)
        det, labels = self.get_bboxes(*outs, img_metas=img_metas, rescale=rescale)
        det, labels = det.cpu().numpy(), labels.cpu().numpy()
        return [self.bbox2result(det[i], labels[i], self.num_classes) for i in range(len(img_metas))]

    simple_test_bboxes = simple_test

    def _get_bboxes_single(self, *a, **k):
        raise NotImplementedError("the batch form: get_bboxes()")
