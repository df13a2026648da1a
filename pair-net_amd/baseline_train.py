"""One training iteration of the sibling head `CrossHeadBaseline` ("PSGFormer+",
configs/mask2former/baseline_r50_psg.py) on the MI355X: the reference's `forward_train` -> `loss` ->
`losses.backward()` -> clip -> AdamW step for every parameter that backward pass reaches -- the
relation branch, the class / mask heads and the nine masked decoder layers (`BaselineHeadGrad`), the
pixel decoder with its FPN branch (`SegPixelDecoderGrad`) and, with `backbone=`, the ResNet's stages
2-4 (`BackboneGrad`; stem, layer1 and BatchNorm frozen, `frozen_stages=1`).

    trainer = BaselineTrainer(head)                  # or BaselineTrainer(head, backbone=resnet)
    out = trainer.step(feats, img_metas, gt_rels, gt_labels, gt_masks)     # feats, or the image

Per step: the backbone (if given) -> `head.forward` with all decoder layers -> `head.full_losses`
(the 30 terms and six logit gradients; targets built on the device) -> the three tapes' forward and
backward in `CrossHeadBaseline.full_backward`'s order, then `BackboneGrad` on d C3 / C4 / C5, all into
ONE flat gradient buffer [BaselineHeadGrad | SegPixelDecoderGrad | BackboneGrad] -> clip, one guarded
AdamW launch, refresh of every derived pack (`FlatTrainer`, flat_trainer.py: the flat buffers, their
set-up and everything behind the backward pass).  `step` holds no host wait: the two assignment
status words (`seg_status()`, `rel_status()`) are OR-ed on the device into the AdamW launch's guard, so a refused assignment moves
no parameter and the host never looks; `step` returns the word as `assign_status`.  (A batch whose
sides exceed `hip.LSA_MAX_SIDE` takes the loss objects' host path, as everywhere.)  The host counter
`steps` advances on a skipped step too, as `TailTrainer`'s does.

Nothing is frozen in the layout: `cls_embed` and `post_norm` carry loss terms in this head.
`relation_decoder.post_norm.*` is not in it: the reference's forward never applies that module, so
autograd reaches no gradient for it (labnotes R23.1).

Optimizer groups (baseline_r50_psg.py:535-550): `paramwise_cfg.custom_keys` gives `backbone`,
`transformer_decoder`, `pixel_decoder` and `decoder_input_projs` lr_mult = 0.1 and decay_mult = 0.1
each; `norm_decay_mult = 0`.  The rule applied here: a parameter whose name contains a key takes
that key's two multipliers and nothing else; otherwise a normalisation layer's parameter takes
`norm_decay_mult` on its decay; everything else takes 1.  UNPINNED: this rule is restated from
memory of mmcv's `DefaultOptimizerConstructor` (mmcv does not import where this was written, so no
test holds it to mmcv), and so is the schedule of `set_epoch` (`lr_config = dict(policy="step",
step=40)` with mmcv's default gamma 0.1).

Deliberately out:
  * the relation decoder's train-mode `ffn_drop = 0.1`: the step is deterministic
    (`BaselineHeadGrad.forward_from_plan(dropout=)` exists; the loss would have to see its outputs);
  * `reduce_mean` across ranks: the caller passes `num_total_masks`;
  * `GradReducer` / `group=`: the tapes' `on_ready` ends are monotone over the one buffer
    (`last_ready_ends`), so a reducer can be attached later;
  * `SeesawLoss`;
  * the pixel-decoder tape's exact-fp32 operating point: the known limitation of
    `CrossHeadBaseline.segmenter_backward` stays;
  * a Swin backbone (`NotImplementedError`).
"""
import contextlib

import torch

from . import hip
from .flat_trainer import (FPN_CONV, FlatTrainer, refresh_encoder, refresh_fpn_conv,
                           refresh_key_positions, refresh_q0, refresh_query_positions, refresh_r0,
                           refresh_resnet, refresh_self_attention)
from .backbone_grad import BackboneGrad
from .seg_grad import BaselineHeadGrad, SegPixelDecoderGrad

__all__ = ["SegmenterTrainer", "BaselineTrainer"]

CUSTOM_KEYS = ("backbone", "transformer_decoder", "pixel_decoder", "decoder_input_projs")


class SegmenterTrainer(FlatTrainer):
    """What the trainers of the two heads on the Mask2Former segmenter share (`BaselineTrainer`
    below, `PSGTr2Trainer` in psgtr2_train.py): the layout [head tape | SegPixelDecoderGrad |
    BackboneGrad], the optimizer groups, the step and the refresh of the segmenter's packs.  A
    subclass states its head tape, its default decay multiplier of the custom keys, whether its
    loss reads all decoder layers, and `_check_head`, `_losses`, `_status`, `_refresh_head`."""
    # the default for the head tape's `masked_keysplit_min_keys`: the smallest measured
    # level at and above which pn_mha_bwd_keysplit_masked_f32 beat pn_mha_bwd_f32 in all three
    # repeats for both mask families (tools/baseline_step_probe.py, profiles/baseline_step.json,
    # labnotes R24.4: 0.27 against 0.46 ms at 4 200 keys, 0.74 against 1.73 ms at 16 700, but 0.26
    # against 0.14 ms at 1 050)
    MASKED_KEYSPLIT_MIN_KEYS = 4200
    LR_STEPS, LR_GAMMA = (40,), 0.1    # `lr_config = dict(policy="step", step=40)`, mmcv's default gamma
    HEAD_TAPE, DECAY_MULT, ALL_LAYERS = None, None, False

    def __init__(self, head, backbone, lr, weight_decay, betas, eps, max_norm, lr_mult, decay_mult,
                 norm_decay_mult, seed, masked_keysplit_min_keys, deterministic):
        """`lr_mult` / `decay_mult`: {substring of a parameter name: multiplier} (mmcv's
        `paramwise_cfg.custom_keys`; default: the four keys of the module docstring at 0.1 /
        `DECAY_MULT`); a backbone's parameters appear as "backbone.<name>".
        `masked_keysplit_min_keys`: the head tape's switch (None: `pn_mha_bwd_f32` for all nine
        masked cross-attentions); the default is the measured `MASKED_KEYSPLIT_MIN_KEYS`.
        `deterministic`: the pixel-decoder tape's deformable-attention backward without float
        atomics (`PixelDecoderGrad.deterministic`, `pn_msda_bwd_det_f32`): the whole step is then
        bitwise reproducible."""
        from .swin import SwinTransformerHip
        self._check_head(head)
        if isinstance(backbone, SwinTransformerHip):
            raise NotImplementedError("%s trains a ResNet50Hip backbone (stages 2-4); "
                                      "a Swin backbone is out of scope" % type(self).__name__)
        self.seed = int(seed)
        lr_mult = dict({k: 0.1 for k in CUSTOM_KEYS} if lr_mult is None else lr_mult)
        decay_mult = dict({k: self.DECAY_MULT for k in CUSTOM_KEYS} if decay_mult is None
                          else decay_mult)
        segments = [("tape", "", self.HEAD_TAPE, head), ("pd_tape", "", SegPixelDecoderGrad, head)]
        if backbone is not None:
            segments.append(("bb_tape", "backbone.", BackboneGrad, backbone))
        self.last_ready_ends = []

        def rule(names, frozen):
            pairs = [self.multipliers(n, lr_mult, decay_mult, norm_decay_mult) for n in names]
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

    # ------------------------------------------------------------------
    @staticmethod
    def is_norm(name):
        """Whether `name` (a head parameter, or "backbone.<name>") belongs to a normalisation
        layer: the decoders' LayerNorms, the pixel decoder's GroupNorms, the backbone's BatchNorm."""
        return ".norms." in name or "post_norm" in name or ".gn." in name or ".bn" in name or \
            ".downsample.1." in name

    @staticmethod
    def multipliers(name, lr_mult, decay_mult, norm_decay_mult):
        """(lr multiplier, decay multiplier) of one parameter under the rule of the module
        docstring: the first key contained in the name (longest key first) decides alone."""
        keys = sorted(set(lr_mult) | set(decay_mult), key=lambda k: (-len(k), k))
        for key in keys:
            if key in name:
                return float(lr_mult.get(key, 1.0)), float(decay_mult.get(key, 1.0))
        if SegmenterTrainer.is_norm(name):
            return 1.0, float(norm_decay_mult)
        return 1.0, 1.0

    def _refresh_derived(self):
        """Every weight pack the head's (and the backbone's) INFERENCE kernels read that is a
        function of trained parameters, rewritten in place (captured hipGraphs keep their
        pointers): the decoder's self-attention [V | Q | K] projections, what `_refresh_head`
        adds, the batch-repeated initial queries and their mask embedding, both position tables
        (they carry `level_embed` / `level_encoding`), the encoder's [value | offsets | weights]
        projections and bf16-plane splits, the FPN branch's 3x3 convolution in its direct and two
        Winograd forms, and the backbone's BatchNorm-folded packs.  Everything else the forward
        reads (the class heads, the MLPs, norms, the 1x1 convolutions, `mask_feature`) is a view
        of the flat buffer -- or, for `PSGTrHead2`'s `mask_embed` / `sub_mask_embed`, untrained."""
        head, w, p = self.head, self.head.w, self.params
        refresh_self_attention(head, w, p, "transformer_decoder", head.num_dec_layers, 1)
        self._refresh_head(head, w, p)
        refresh_q0(head, w, p)
        refresh_key_positions(head, w, p)
        refresh_query_positions(head, w, p)
        refresh_encoder(head, w, p)
        refresh_fpn_conv(head, w, p)
        if self.bb_tape is not None:
            refresh_resnet(self.backbone, self.backbone.w, p, self.bb_tape)

    def _refresh_head(self, head, w, p):
        """The head's own packs beyond the segmenter's (default: none; `PSGTrHead2`'s `query_feat`
        and `post_norm` move with `q0`, its `mask_embed` is not trained)."""

    def _gradients_ready(self, end):
        self.last_ready_ends.append(end)       # (no reducer: module docstring)

    # ------------------------------------------------------------------
    @torch.no_grad()
    @hip.on_device
    def step(self, feats, img_metas, gt_rels, gt_labels, gt_masks, num_total_masks=None):
        """One iteration on one batch.  `feats`: the four backbone feature maps -- or, for a
        trainer built with `backbone=`, the image tensor.  `gt_masks` at half the batch tensor's
        size (`PSGTr._prepare_gt_masks`).  Returns the head's loss terms (`_losses`: the 30 of
        `full_losses`, the seven of `triplet_losses`) plus `grad_norm` (before clipping) and
        `assign_status` (int32; non-zero: an assignment was refused and the update was skipped),
        all device scalars."""
        head, tape = self.head, self.tape
        self._check_not_repacked()
        if self.backbone is not None:
            feats = [f.clone(memory_format=torch.preserve_format) for f in self.backbone(feats)]
        with head.all_layers() if self.ALL_LAYERS else contextlib.nullcontext():
            cls, masks = head.forward(feats, img_metas)
        pl = head._last_plan
        up = {}
        losses, counts = self._losses(cls, masks, gt_rels, None, gt_labels, gt_masks, img_metas,
                                      grads=up, seed=self.seed, step=self.steps,
                                      num_total_masks=num_total_masks)
        self.last_ready_ends = []
        tape.forward_from_plan(pl)
        dmem, dMF, _ = tape.backward(up, counts=counts, on_ready=self._ready(0))
        self.pd_tape.forward(feats)
        dfeats, _ = self.pd_tape.backward(dmem, dMF, on_ready=self._ready(1))
        if self.bb_tape is not None:               # dfeats: d C5, d C4, d C3 (, d C2: layer1 is frozen)
            self.bb_tape.forward(feats[0])
            self.bb_tape.backward(dfeats[2], dfeats[1], dfeats[0], on_ready=self._ready(2))
        self._status(out=self._guard)
        self.apply_gradients(guard=self._guard)
        out = dict(losses)
        out["grad_norm"] = self.clip[0]
        out["assign_status"] = self._guard[0]
        return out


class BaselineTrainer(SegmenterTrainer):
    HEAD_TAPE, DECAY_MULT, ALL_LAYERS = BaselineHeadGrad, 0.1, True

    def __init__(self, head, backbone=None, lr=1e-4, weight_decay=1e-4, betas=(0.9, 0.999),
                 eps=1e-8, max_norm=0.1, lr_mult=None, decay_mult=None, norm_decay_mult=0.0, seed=0,
                 masked_keysplit_min_keys="default", deterministic=False):
        """`SegmenterTrainer.__init__` with the defaults of baseline_r50_psg.py."""
        super().__init__(head, backbone, lr, weight_decay, betas, eps, max_norm, lr_mult, decay_mult,
                         norm_decay_mult, seed, masked_keysplit_min_keys, deterministic)

    def _check_head(self, head):
        if not hasattr(head, "_relation_stage") or not hasattr(head, "full_losses"):
            raise NotImplementedError("BaselineTrainer trains a CrossHeadBaseline (%s: TailTrainer)"
                                      % type(head).__name__)

    def _losses(self, *args, **kw):
        """The 30 terms of `full_losses` (targets built on the device) and the matched counts."""
        losses = self.head.full_losses(*args, **kw)
        return losses, self.head._seg_loss.last["counts"]

    def _status(self, out):
        head = self.head          # both assignment status words, OR-ed on the device
        torch.bitwise_or(head.seg_status().view(1), head.rel_status().view(1), out=out)

    def _refresh_head(self, head, w, p):
        """The relation decoder's self-attention packs and its batch-repeated initial queries."""
        refresh_self_attention(head, w, p, "relation_decoder", head.num_rel_layers, 0)  # self-first
        refresh_r0(head, w, p)
