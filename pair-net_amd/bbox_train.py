"""One training iteration of `CrossHeadBBox` on the MI355X: the reference's `forward_train` ->
`loss` -> `backward` -> clip -> AdamW step (pairnet_bbox_head.py:968-1006, :362-464;
configs/deformable_detr/cross_r101_vg.py:307-324) for the parameters the reference's graph reaches.

That graph is short.  `forward` detaches everything the trunk produces (`query_feats =
hs.clone().detach()`, pairnet_bbox_head.py:261; `cls_pred.clone().detach()`, :322-330) and `loss`
has its detection terms commented out (:362-464, :596-642), so `losses.backward()` reaches only
`sub_query_update` / `obj_query_update`, `update_importance`, the six `relation_decoder` layers,
`rel_query_feat`, `rel_query_pos_embed`, `rel_key_pos_embed` and `rel_cls_embed` (10.2 M) -- the
trunk, neck and backbone get `.grad = None`, which is why the config sets
`find_unused_parameters=True`.  Parameters without a gradient are not in the flat buffer: AdamW
neither decays nor moves them (torch skips a parameter whose `.grad` is None).

    trainer = BBoxTrainer(head)                        # AdamW(lr=2e-4, wd=1e-4), clip 0.1
    losses = trainer.step(feats, img_metas, gt_rels, gt_bboxes, gt_labels)

Per step:
  1. trunk up to `_select` (encoder, two-stage proposals, decoder, query ranking): the inference
     kernels, eval mode, no tape; the backbone and neck run before it (`PSGTr.box_train_step`);
  2. `BBoxTailGrad.forward` from the kept, detached queries `pl.q` and class logits `pl.cls`;
  3. `head.loss(..., grads=)` (bbox_losses.py: `pn_box_match_cost_f32`, the two assignments);
  4. the tape's backward into the flat gradient buffer;
  5. `FlatTrainer.apply_gradients` (flat_trainer.py, which also owns the buffers and their
     set-up): global-norm clip (`max_norm`, default 0.1; cross_r101_vg.py:324 itself sets 0.01),
     ONE AdamW launch -- `device_targets=True`: the guarded launch behind `assign_status`, no
     host wait in `step()` -- and the refresh of the relation stage's derived packs.

DETERMINISTIC.  The reference runs the trunk in train mode, so its 0.1 dropouts (the decoder's
self-attention and every FFN of the trunk, cross_r101_vg.py:41-80) are drawn even though nothing
flows back through them: its kept queries are those of a randomly thinned trunk.  This step runs
the trunk in eval mode and draws nothing: two runs from the same state give the same bits.  The
relation decoder's own rates are 0 in the config.

Out of scope: the one-stage / no-refine trunk, the RMSNorm / SwiGLU decoder of
`pairnet_r101_vg.py` and its MultilabelFocalLoss, the commented-out detection losses, a
data-parallel `group=` step, training the trunk, neck or backbone (the graph does not reach them).
"""
import torch

from . import hip
from . import plans
from .dist import GradReducer
from .flat_trainer import (MATRIX_LEARNER_REPACKED, FlatTrainer, refresh_matrix_learner, refresh_r0,
                           refresh_relation_cross_attention, refresh_self_attention)
from .grad import BBoxTailGrad
from .train import segment_multipliers

__all__ = ["BBoxTrainer"]


class BBoxTrainer(FlatTrainer):
    """`FlatTrainer` around `BBoxTailGrad` (module docstring); nothing in its layout is frozen."""

    def __init__(self, head, lr=2e-4, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 max_norm=0.1, norm_decay_mult=0.0, lr_mult=None, decay_mult=None,
                 device_targets=False):
        from .bbox_head import CrossHeadBBox
        if not isinstance(head, CrossHeadBBox):
            raise TypeError("BBoxTrainer trains a CrossHeadBBox (TailTrainer: CrossHead2, "
                            "BaselineTrainer: CrossHeadBaseline)")
        self.device_targets = bool(device_targets)
        if head.device is None or head.device.type != "cuda":
            raise RuntimeError("BBoxTrainer needs a head on an MI355X (.to('cuda:N'))")
        super().__init__(
            head, [("tape", "", BBoxTailGrad, head)],
            lambda names, frozen: segment_multipliers(names, frozen, lr_mult, decay_mult,
                                                      norm_decay_mult),
            lr=lr, weight_decay=weight_decay, betas=betas, eps=eps, max_norm=max_norm,
            repacked=MATRIX_LEARNER_REPACKED,
            aliases=BBoxTailGrad.ALIASES)       # CrossHead2's names of the relation stage
        self.reducer = GradReducer(self.flat_grad, group=None)

    def _refresh_derived(self):
        """The packs `CrossHeadBBox._pack` builds for the relation stage."""
        head, w, p = self.head, self.head.w, self.params
        refresh_self_attention(head, w, p, "relation_decoder", head.num_rel_layers, 1)
        refresh_relation_cross_attention(head, w, p)
        refresh_matrix_learner(head, w, p)
        refresh_r0(head, w, p)

    def _trunk(self, feats, img_metas):
        """Step 1: the inference kernels up to `_select` -> the plan (pl.q, pl.cls, pl.box)."""
        head = self.head
        B, shapes, _ = head._check_feats(feats, img_metas)
        pl = head._plan(B, shapes, None, 0)
        head._run_stage("a", pl, feats)
        cur = torch.cuda.current_stream(self.dev)
        try:
            head._decoder(pl)
            head._select(pl)
        finally:
            plans.note_use(cur)
        head._last_plan = pl
        return pl

    @torch.no_grad()
    @hip.on_device
    def step(self, feats, img_metas, gt_rels, gt_bboxes, gt_labels):
        """One iteration on one batch of neck features; returns the four loss terms (device
        scalars, as `CrossHeadBBox.loss`) plus `grad_norm` (before clipping) and, for a
        `device_targets` trainer, `assign_status` (device int32 scalar; non-zero: the batch's cost
        matrices were refused and the update was skipped on the device)."""
        head, tape = self.head, self.tape
        self._check_not_repacked()
        pl = self._trunk(feats, img_metas)
        out = tape.forward(pl.q, pl.cls)
        up = {}
        losses = head.loss(dict(cls=pl.cls, sub=out["sub"], obj=out["obj"], rel=out["rel"],
                                importance=out["importance"]), dict(bbox=pl.box), gt_rels,
                           gt_bboxes, gt_labels, img_metas, grads=up,
                           device_targets=self.device_targets)
        self.reducer.start()
        tape.backward(g_rel=up["rel"], g_importance=up["importance"], on_ready=self._ready(0))
        self.reducer.finish()
        guard = head._loss.assign_status if self.device_targets else None
        self.apply_gradients(guard=guard)
        res = dict(losses)
        res["grad_norm"] = self.clip[0]
        if self.device_targets:
            res["assign_status"] = guard[0]
        return res
