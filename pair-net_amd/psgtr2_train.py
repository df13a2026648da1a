"""One training iteration of `PSGTrHead2` ("PSGTR on Mask2Former",
configs/psgtr/psgtr_r50_psg_plus.py) on the MI355X: the reference's `forward_train` -> `loss` ->
`losses.backward()` -> clip -> AdamW step for every parameter that backward pass reaches -- the three
class heads, `obj_mask_embed`, `post_norm` and the nine masked decoder layers (`PSGTr2HeadGrad`), the
pixel decoder with its FPN branch (`SegPixelDecoderGrad`) and, with `backbone=`, the ResNet's stages
2-4 (`BackboneGrad`; stem, layer1 and BatchNorm frozen, `frozen_stages=1`).

    trainer = PSGTr2Trainer(head)                    # or PSGTr2Trainer(head, backbone=resnet)
    out = trainer.step(feats, img_metas, gt_rels, gt_labels, gt_masks)     # feats, or the image

Per step: the backbone (if given) -> `head.forward` -> `head.triplet_losses` (the seven terms and six
logit gradients; triplet matching on the device) -> the tapes' forward and backward in
`PSGTrHead2.triplet_backward`'s order, then `BackboneGrad` on d C3 / C4 / C5, all into ONE flat
gradient buffer [PSGTr2HeadGrad | SegPixelDecoderGrad | BackboneGrad] -> clip, one guarded AdamW
launch, refresh of every derived pack (`FlatTrainer`, flat_trainer.py).  `step` holds no host wait:
the assignment status word (`head.triplet_status()`) is the AdamW launch's guard, so a refused
assignment moves no parameter and the host never looks; `step` returns the word as `assign_status`.
(A batch whose sides exceed `hip.LSA_MAX_SIDE` takes the loss object's host path, as everywhere.)
The host counter `steps` advances on a skipped step too.

`mask_embed.*` and `sub_mask_embed.*` are not in the layout: the reference's autograd leaves both at
`grad is None` (the first feeds only the detached attention masks, the second reaches no output), so
its optimizer neither decays nor moves them, and neither does this step.

Optimizer groups (psgtr_r50_psg_plus.py:299-317): lr 1e-4, weight decay 1e-4, `grad_clip` max_norm
0.1; `paramwise_cfg.custom_keys` gives `backbone`, `transformer_decoder`, `pixel_decoder` and
`decoder_input_projs` lr_mult = 0.1 and decay_mult = 1.0 each; no `norm_decay_mult` (1.0).  The rule
is `BaselineTrainer.multipliers` (baseline_train.py): a parameter whose name contains a key takes
that key's two multipliers and nothing else; otherwise a normalisation layer's parameter takes
`norm_decay_mult` on its decay; everything else takes 1.  UNPINNED: that rule is restated from memory
of mmcv's `DefaultOptimizerConstructor` (no test holds it to mmcv), and so is the schedule of
`set_epoch` (`lr_config = dict(policy="step", step=40)` with mmcv's default gamma 0.1).

All dropout rates of this config are 0: the step draws nothing but the loss's points.

Deliberately out: `reduce_mean` across ranks (the caller passes `num_total_masks`); `GradReducer` /
`group=` (the tapes' `on_ready` ends are monotone over the one buffer, `last_ready_ends`); a Swin
backbone (`NotImplementedError`); `HTriMatcher`, `use_mask=False`; the pixel-decoder tape's
exact-fp32 operating point (the known limitation of `triplet_backward` stays).
"""
from .baseline_train import SegmenterTrainer
from .seg_grad import PSGTr2HeadGrad

__all__ = ["PSGTr2Trainer"]


class PSGTr2Trainer(SegmenterTrainer):
    # (the same kernel at the same memory levels as `BaselineTrainer`'s head tape, labnotes R24.4:
    # `MASKED_KEYSPLIT_MIN_KEYS` is the base's)
    HEAD_TAPE, DECAY_MULT, ALL_LAYERS = PSGTr2HeadGrad, 1.0, False

    def __init__(self, head, backbone=None, lr=1e-4, weight_decay=1e-4, betas=(0.9, 0.999),
                 eps=1e-8, max_norm=0.1, lr_mult=None, decay_mult=None, norm_decay_mult=1.0, seed=0,
                 masked_keysplit_min_keys="default", deterministic=False):
        """`SegmenterTrainer.__init__` with the defaults of psgtr_r50_psg_plus.py."""
        super().__init__(head, backbone, lr, weight_decay, betas, eps, max_norm, lr_mult, decay_mult,
                         norm_decay_mult, seed, masked_keysplit_min_keys, deterministic)

    def _check_head(self, head):
        if not hasattr(head, "triplet_losses") or not hasattr(head, "triplet_backward"):
            raise NotImplementedError("PSGTr2Trainer trains a PSGTrHead2 (%s: TailTrainer / "
                                      "BaselineTrainer / BBoxTrainer)" % type(head).__name__)

    def _losses(self, *args, **kw):
        """The seven terms of `triplet_losses` (triplet matching on the device) and the counts."""
        losses = self.head.triplet_losses(*args, **kw)
        return losses, self.head._tri_loss.last["counts"]

    def _status(self, out):
        out.copy_(self.head.triplet_status().view(1))
