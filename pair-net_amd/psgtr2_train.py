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
import torch

from . import hip
from .baseline_train import CUSTOM_KEYS, BaselineTrainer
from .flat_trainer import (FPN_CONV, FlatTrainer, refresh_encoder, refresh_fpn_conv,
                           refresh_key_positions, refresh_q0, refresh_query_positions,
                           refresh_resnet, refresh_self_attention)
from .backbone_grad import BackboneGrad
from .seg_grad import PSGTr2HeadGrad, SegPixelDecoderGrad

__all__ = ["PSGTr2Trainer"]


class PSGTr2Trainer(FlatTrainer):
    # the same kernel at the same memory levels as `BaselineTrainer`'s head tape (labnotes R24.4)
    MASKED_KEYSPLIT_MIN_KEYS = BaselineTrainer.MASKED_KEYSPLIT_MIN_KEYS
    LR_STEPS, LR_GAMMA = (40,), 0.1    # `lr_config = dict(policy="step", step=40)`, mmcv's default gamma

    def __init__(self, head, backbone=None, lr=1e-4, weight_decay=1e-4, betas=(0.9, 0.999),
                 eps=1e-8, max_norm=0.1, lr_mult=None, decay_mult=None, norm_decay_mult=1.0, seed=0,
                 masked_keysplit_min_keys="default", deterministic=False):
        """`lr_mult` / `decay_mult`: {substring of a parameter name: multiplier} (mmcv's
        `paramwise_cfg.custom_keys`; default: the four keys of the module docstring at 0.1 / 1.0); a
        backbone's parameters appear as "backbone.<name>".  `masked_keysplit_min_keys`: the head
        tape's switch (None: `pn_mha_bwd_f32` for all nine masked cross-attentions); the default
        is `MASKED_KEYSPLIT_MIN_KEYS`.  `deterministic`: the pixel-decoder tape's deformable-attention
        backward without float atomics: the whole step is then bitwise reproducible."""
        from .swin import SwinTransformerHip
        if not hasattr(head, "triplet_losses") or not hasattr(head, "triplet_backward"):
            raise NotImplementedError("PSGTr2Trainer trains a PSGTrHead2 (%s: TailTrainer / "
                                      "BaselineTrainer / BBoxTrainer)" % type(head).__name__)
        if isinstance(backbone, SwinTransformerHip):
            raise NotImplementedError("PSGTr2Trainer trains a ResNet50Hip backbone (stages 2-4); "
                                      "a Swin backbone is out of scope")
        self.seed = int(seed)
        lr_mult = dict({k: 0.1 for k in CUSTOM_KEYS} if lr_mult is None else lr_mult)
        decay_mult = dict({k: 1.0 for k in CUSTOM_KEYS} if decay_mult is None else decay_mult)
        segments = [("tape", "", PSGTr2HeadGrad, head), ("pd_tape", "", SegPixelDecoderGrad, head)]
        if backbone is not None:
            segments.append(("bb_tape", "backbone.", BackboneGrad, backbone))
        self.last_ready_ends = []

        def rule(names, frozen):
            pairs = [BaselineTrainer.multipliers(n, lr_mult, decay_mult, norm_decay_mult)
                     for n in names]
            return [lm for lm, _ in pairs], [dm for _, dm in pairs]

        # (nothing in the layout is frozen; the FPN 3x3 convolution's w[...] holds another layout)
        super().__init__(
            head, segments, rule, backbone=backbone, lr=lr, weight_decay=weight_decay, betas=betas,
            eps=eps, max_norm=max_norm, repacked=(FPN_CONV + "weight",))
        self.tape.masked_keysplit_min_keys = self.MASKED_KEYSPLIT_MIN_KEYS \
            if isinstance(masked_keysplit_min_keys, str) and masked_keysplit_min_keys == "default" \
            else masked_keysplit_min_keys
        self.deterministic = bool(deterministic)
        self.pd_tape.deterministic = self.deterministic
        self._guard = torch.zeros(1, device=self.dev, dtype=torch.int32)

    def _refresh_derived(self):
        """Every weight pack this head's (and the backbone's) INFERENCE kernels read that is a
        function of trained parameters, rewritten in place: the decoder's self-attention
        [V | Q | K] projections, the batch-repeated initial queries and their `mask_embed` row pack
        (`query_feat` and `post_norm` move, `mask_embed` does not), both position tables, the
        encoder's packs, the FPN branch's 3x3 convolution in its three forms and the backbone's
        BatchNorm-folded packs.  Everything else the forward reads is a view of the flat buffer
        (or, for `mask_embed` / `sub_mask_embed`, untrained)."""
        head, w, p = self.head, self.head.w, self.params
        refresh_self_attention(head, w, p, "transformer_decoder", head.num_dec_layers, 1)
        refresh_q0(head, w, p)
        refresh_key_positions(head, w, p)
        refresh_query_positions(head, w, p)
        refresh_encoder(head, w, p)
        refresh_fpn_conv(head, w, p)
        if self.bb_tape is not None:
            refresh_resnet(self.backbone, self.backbone.w, p, self.bb_tape)

    def _gradients_ready(self, end):
        self.last_ready_ends.append(end)       # (no reducer: module docstring)

    # ------------------------------------------------------------------
    @torch.no_grad()
    @hip.on_device
    def step(self, feats, img_metas, gt_rels, gt_labels, gt_masks, num_total_masks=None):
        """One iteration on one batch.  `feats`: the four backbone feature maps -- or, for a
        trainer built with `backbone=`, the image tensor.  `gt_masks` at half the batch tensor's
        size (`PSGTr._prepare_gt_masks`).  Returns the seven loss terms of `triplet_losses` plus
        `grad_norm` (before clipping) and `assign_status` (int32; non-zero: the assignment was
        refused and the update was skipped), all device scalars."""
        head, tape = self.head, self.tape
        self._check_not_repacked()
        if self.backbone is not None:
            feats = [f.clone(memory_format=torch.preserve_format) for f in self.backbone(feats)]
        cls, masks = head.forward(feats, img_metas)
        pl = head._last_plan
        up = {}
        losses = head.triplet_losses(cls, masks, gt_rels, None, gt_labels, gt_masks, img_metas,
                                     grads=up, seed=self.seed, step=self.steps,
                                     num_total_masks=num_total_masks)
        self.last_ready_ends = []
        tape.forward_from_plan(pl)
        dmem, dMF, _ = tape.backward(up, counts=head._tri_loss.last["counts"],
                                     on_ready=self._ready(0))
        self.pd_tape.forward(feats)
        dfeats, _ = self.pd_tape.backward(dmem, dMF, on_ready=self._ready(1))
        if self.bb_tape is not None:               # dfeats: d C5, d C4, d C3 (, d C2: layer1 is frozen)
            self.bb_tape.forward(feats[0])
            self.bb_tape.backward(dfeats[2], dfeats[1], dfeats[0], on_ready=self._ready(2))
        self._guard.copy_(head.triplet_status().view(1))
        self.apply_gradients(guard=self._guard)
        out = dict(losses)
        out["grad_norm"] = self.clip[0]
        out["assign_status"] = self._guard[0]
        return out
