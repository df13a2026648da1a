"""One training iteration of Pair-Net's own parameters on the MI355X: the
reference's `forward_train` -> `loss` -> `backward` -> clip -> AdamW step (frameworks/psgtr.py:112-146,
pairnet_head.py:419-757, tools/train.py:115-241, configs/mask2former/pairnet.py:353-368) for the
parameters of `CrossHead2` the loss reaches: by default the Relation Fusion decoder,
`rel_cls_embed`, the relation query / position embeddings, the Pair Proposal Network's MLPs and the
Matrix Learner (10.2 M), with `train_decoder` the nine masked decoder layers as well (+14.3 M) and
with `train_pixel_decoder` the pixel decoder's encoder path (+5.3 M), with `backbone=` the ResNet's
stages 2-4 (+23.2 M; stem, layer1 and BatchNorm frozen as in the reference's config) -- 53.0 M, the
reference's whole trainable graph.  With a `SwinTransformerHip` as `backbone=` the last stage and
its output norm train instead (`SwinBackboneGrad`; `frozen_stages=3` as in
configs/mask2former/pairnet_swinb.py:220: 25.2 M for Swin-B, 56.7 M for Swin-L); one whose
`frozen_stages` is lower trains every stage from there down -- with -1 also every patch merging and
the patch embedding, as configs/deformable_detr/cross_swinb_vg.py:202-226 does (`SwinStagesGrad`,
taped from the image).  Without `backbone=` the backbone is frozen (a fine-tuning regime).
Everything the reference's loss can reach enters through two logits: `loss_r_cls` through
`rel`, `loss_match` through `importance` (`loss_sub_cls` / `loss_obj_cls` read DETACHED class
logits, pairnet_head.py:380-390, and train nothing).

    trainer = TailTrainer(head)                       # AdamW(lr=1e-4, wd=1e-4), clip 0.1
    losses = trainer.step(feats, img_metas, gt_rels, gt_labels, gt_masks)

Per step: `head.forward` (the inference kernels; hipGraphs if on) -> `head.loss(grads=)` (csrc/
loss.hip; the two Hungarian assignments on the host as the reference) -> `RelationTailGrad`
(/ `HeadGrad` / `PixelDecoderGrad` / `BackboneGrad` / `SwinBackboneGrad` / `SwinStagesGrad`) forward-with-tape + backward into one flat
gradient buffer -> (world > 1) bucketed all-reduce
overlapped with the backward pass (`dist.GradReducer`) -> clip, ONE AdamW launch, refresh of the
derived weight packs (`FlatTrainer`, flat_trainer.py: the flat buffers, their set-up and everything
behind the backward pass are shared with the other two training steps).  No host synchronisation
inside a step apart from the reference's own (the Hungarian cost matrices).

`TailTrainer(head, device_targets=True)` removes that one too: the assignments and the target
bookkeeping run on the device (`head.loss(..., device_targets=True)`, csrc/assign.hip) and `step()`
contains no host wait at all -- same losses, same parameters, bit for bit.  What the host path
raises on (a NaN / -inf / infeasible cost matrix, before any parameter moves) the device path
cannot raise without looking: `step()` returns `assign_status` (a device word) and the AdamW launch
is the guarded one (`pn_adamw_guarded_f32`), which returns early on a non-zero status, so
`flat_p` / `flat_m` / `flat_v` stay bitwise unchanged.  The host step counter `steps` still
advances on such a step (the host does not know), and with it the bias corrections' exponent and
the dropout draws' key: a skipped batch uses up its step number.  The status word is per rank:
under `group=` the other ranks do not see it (their all-reduced gradient carries the bad rank's
NaN), so a data-parallel loop should read `assign_status` and stop, as the host path's exception
does.

Dropout.  The reference's config has ONE non-zero dropout rate, the Relation Fusion decoder's
`ffn_drop=0.1` (configs/mask2former/pairnet.py:126): mmcv's FFN drops the hidden rows after the ReLU
and the FFN's output before the shortcut, twelve `nn.Dropout` per iteration.  It is off by default
(the deterministic step described above, launch for launch); `TailTrainer(head, dropout=True)`
honours the configured rate (a float overrides it).  The taped forward then runs BEFORE the loss
with the two dropouts per layer (csrc/dropout.hip: Philox4x32-10 keyed by `seed`, counter = (element
/ 4, rank in `group`, site = 2 * layer + {0, 1}, `self.steps`); no mask stored, nothing uploaded),
`head.loss` is handed the tape's dropped `rel` in place of the inference kernels' -- so `loss_r_cls`
and d loss / d rel are those of the dropped logits, and nothing else of the outputs changes -- and
the backward pass re-draws the same masks from the same counter.  The inference path never drops.
"""
import torch

from . import hip
from .dist import GradReducer
from .flat_trainer import (MATRIX_LEARNER_REPACKED, FlatTrainer, refresh_encoder,
                           refresh_key_positions, refresh_matrix_learner, refresh_q0,
                           refresh_query_positions, refresh_r0, refresh_relation_cross_attention,
                           refresh_resnet, refresh_self_attention, refresh_swin, step_lr)
from .backbone_grad import BackboneGrad, SwinBackboneGrad, SwinStagesGrad
from .grad import FfnDropout, HeadGrad, RelationTailGrad
from .pixel_grad import PixelDecoderGrad

__all__ = ["TailTrainer", "step_lr", "segment_multipliers"]


def segment_multipliers(names, frozen, lr_mult=None, decay_mult=None, norm_decay_mult=0.0,
                        swin=False):
    """Per-segment (lr multipliers, weight-decay multipliers) of the flat parameter buffer, mmcv's
    `paramwise_cfg`: `lr_mult` / `decay_mult` {substring of a parameter name: multiplier} (a key
    hit decides alone), `norm_decay_mult` for the head's norms, 0 / 0 for a `frozen` name."""
    lr_mult, decay_mult = dict(lr_mult or {}), dict(decay_mult or {})
    lrs, wds = [], []
    for n in names:
        lrs.append(0.0 if n in frozen else
                   next((m for key, m in lr_mult.items() if key in n), 1.0))
        # (a Swin backbone's names -- norm1 / norm2 / norm3, the bias table -- match none of
        # these: with a `backbone.` custom key mmcv applies no norm_decay_mult to them)
        is_norm = ".norms." in n or "post_norm" in n or ".gn." in n
        assert not (is_norm and swin and n.startswith("backbone.")), n
        wds.append(0.0 if n in frozen else
                   next((m for key, m in decay_mult.items() if key in n),
                        norm_decay_mult if is_norm else 1.0))
    return lrs, wds


class TailTrainer(FlatTrainer):
    FROZEN_GROUPS = ("cls",)      # cls_embed / post_norm: no gradient in the reference's graph
    # `CrossHead2Loss` draws its mask points with `torch.rand(device=)` unless `point_coords=` is
    # given: the device's default generator is part of a run's state (`FlatTrainer.state_dict`)
    DEFAULT_GENERATORS = ("device",)

    def __init__(self, head, lr=1e-4, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 max_norm=0.1, norm_decay_mult=0.0, lr_mult=None, group=None,
                 bucket_bytes=32 << 20, train_decoder=False, train_pixel_decoder=False,
                 backbone=None, drop_path=False, seed=0, dropout=False, device_targets=False,
                 decay_mult=None, deterministic=False):
        """`train_decoder`: also train the nine masked decoder layers, `query_feat`, `query_embed`
        and `level_embed` (`HeadGrad`; the reference's `transformer_decoder` group, lr_mult 0.1 by
        default here as in configs/mask2former/pairnet.py:358-363) -- everything of the head behind
        the pixel decoder.  `lr_mult`: {substring of a parameter name: multiplier} (mmcv's
        `paramwise_cfg.custom_keys`).  `decay_mult`: the same for the weight decay (None: 1 for
        every tensor but the head's norms, as before; {"backbone.": 0.0} is
        configs/deformable_detr/cross_swinb_vg.py:564).  A key hit decides alone (a rule not pinned
        to mmcv's, as for `lr_mult`).  `deterministic`: the pixel-decoder tape's deformable-
        attention backward without float atomics (`PixelDecoderGrad.deterministic`,
        `pn_msda_bwd_det_f32`): the whole step is then bitwise reproducible; without a
        pixel-decoder tape the keyword changes nothing."""
        # `device_targets`: loss targets built on the device, a guarded update, no host wait in
        # `step()` (module docstring); default off: the host assignments, launch for launch
        self.device_targets = bool(device_targets)
        # `backbone` (a ResNet50Hip): also train its stages 2-4 (`BackboneGrad`; the reference's
        # `backbone` group at lr_mult 0.1, stem / layer1 / BatchNorm frozen as in its config):
        # `step()` then takes the IMAGE tensor.  Its parameters appear as "backbone.<name>".
        # A SwinTransformerHip trains its last stage + norm (`SwinBackboneGrad`) at lr_mult 0.01
        # (pairnet_swinb.py:563-571); `drop_path`: mmdet's DropPath on that stage's residual
        # branches at the rates of the backbone's `drop_path_rate`, drawn per step from a host
        # generator seeded with `seed` (default off: a deterministic step).  A Swin backbone with
        # `frozen_stages` below the last stage trains every stage from there down
        # (`SwinStagesGrad`; DropPath then on every trainable block).
        from .swin import SwinTransformerHip
        self.swin = isinstance(backbone, SwinTransformerHip)
        self.drop_path = bool(drop_path) and self.swin
        self._gen = torch.Generator().manual_seed(int(seed))
        # `dropout`: the Relation Fusion decoder's FFN dropout in train mode (mmcv FFN.layers' two
        # nn.Dropout per layer; the reference's config sets ffn_drop=0.1 there and 0.0 everywhere
        # else).  True: the configured rate (`head.rel_ffn_drop`); a float overrides it; False /
        # 0.0 (default): the deterministic step, without a single extra launch.  The masks are
        # drawn on the device by a counter-based generator (csrc/dropout.hip) from (`seed`, the
        # rank in `group`, the step count, the site): nothing is stored or uploaded, ranks draw
        # different masks from one seed, and a restored step count reproduces them.
        self.seed = int(seed)
        self.drop_p = self._dropout_rate(head, dropout)
        import torch.distributed as dist
        ini = dist.is_available() and dist.is_initialized()      # (as GradReducer reads `group`)
        self.subseq = int(dist.get_rank(group)) if ini else 0
        self.train_pixel_decoder = bool(train_pixel_decoder) or backbone is not None
        self.train_decoder = bool(train_decoder) or self.train_pixel_decoder
        if lr_mult is None:
            lr_mult = {"transformer_decoder": 0.1, "pixel_decoder": 0.1,
                       "backbone.": 0.01 if self.swin else 0.1}
        self.swin_stages = self.swin and backbone.frozen_stages < len(backbone.depths) - 1
        tape_cls = HeadGrad if self.train_decoder else RelationTailGrad
        bb_cls = (SwinStagesGrad if self.swin_stages else SwinBackboneGrad) if self.swin \
            else BackboneGrad
        segments = [("tape", "", tape_cls, head)]
        if self.train_pixel_decoder:
            segments.append(("pd_tape", "", PixelDecoderGrad, head))
        if backbone is not None:
            segments.append(("bb_tape", "backbone.", bb_cls, backbone))
        # the class path (cls_embed / post_norm: no gradient in the reference's graph) stays in
        # the layout with lr 0
        frozen = {n for g, names in tape_cls.param_groups(head) if g in self.FROZEN_GROUPS
                  for n in names}
        if self.swin_stages:      # norm0: the loss does not reach C2 -- no gradient, no decay
            frozen |= {"backbone." + n for g, names in bb_cls.param_groups(backbone)
                       if g in bb_cls.NO_GRAD_GROUPS for n in names}
        super().__init__(
            head, segments,
            lambda names, frozen: segment_multipliers(names, frozen, lr_mult, decay_mult,
                                                      norm_decay_mult, swin=self.swin),
            backbone=backbone, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps,
            max_norm=max_norm, frozen=frozen, repacked=MATRIX_LEARNER_REPACKED)
        self.deterministic = bool(deterministic)
        if self.pd_tape is not None:
            self.pd_tape.deterministic = self.deterministic
        self.reducer = GradReducer(self.flat_grad, group=group, bucket_bytes=bucket_bytes)

    # ------------------------------------------------------------------
    @staticmethod
    def _dropout_rate(head, dropout):
        """The rate `dropout=` asks for; True reads the head's config and refuses one whose other
        non-zero rates this step cannot honour."""
        if dropout is True:
            other = head.other_drop_rates
            if other:
                raise NotImplementedError(
                    "dropout=True: the training step drops in the relation decoder's FFN only, but "
                    "the config also sets " + ", ".join("%s=%g" % kv for kv in other.items()))
            return float(head.rel_ffn_drop)
        if dropout is False or dropout is None:
            return 0.0
        p = float(dropout)
        if not 0.0 <= p < 1.0:
            raise ValueError("dropout rate %r outside [0, 1)" % (dropout,))
        return p

    def dropout_descriptor(self, step=None):
        """The `FfnDropout` of iteration `step` (default: the next one), or None when off."""
        if self.drop_p == 0.0:
            return None
        return FfnDropout(self.drop_p, self.seed, self.subseq,
                          self.steps if step is None else step)

    def _refresh_derived(self):
        """The packs of what this trainer trains (flat_trainer.py); both decoders are
        cross-attention first: their self-attention is `attentions.1`."""
        head, w, p = self.head, self.head.w, self.params
        refresh_self_attention(head, w, p, "relation_decoder", head.num_rel_layers, 1)
        refresh_relation_cross_attention(head, w, p)
        refresh_matrix_learner(head, w, p)
        refresh_r0(head, w, p)
        if self.train_decoder:
            refresh_self_attention(head, w, p, "transformer_decoder", head.num_dec_layers, 1)
            refresh_q0(head, w, p)
            refresh_key_positions(head, w, p)
        if self.train_pixel_decoder:
            refresh_encoder(head, w, p)
            refresh_query_positions(head, w, p)
        if self.bb_tape is not None:
            (refresh_swin if self.swin else refresh_resnet)(self.backbone, self.backbone.w, p,
                                                            self.bb_tape)

    def _drop_path_keep(self, B):
        """mmdet DropPath's per-image scale factors [blocks, 2 branches, B] of the trained stage:
        floor(keep_prob + U[0, 1)) / keep_prob at the block's rate of linspace(0, drop_path_rate,
        sum(depths)).  A `SwinStagesGrad` trainer draws them for all sum(depths) blocks (the tape
        ignores the rows of frozen stages)."""
        bb = self.backbone
        S = 0 if self.swin_stages else len(bb.depths) - 1
        dpr = torch.linspace(0, bb.drop_path_rate, sum(bb.depths), dtype=torch.float64)
        rates = dpr[sum(bb.depths[:S]):].float()                          # [blocks]
        kp = (1.0 - rates).view(-1, 1, 1)
        u = torch.rand(len(rates), 2, B, generator=self._gen)
        keep = torch.floor(kp + u) / kp
        return keep.pin_memory().to(self.dev, non_blocking=True) if torch.cuda.is_available() \
            else keep

    # ------------------------------------------------------------------
    @torch.no_grad()
    @hip.on_device
    def step(self, feats, img_metas, gt_rels, gt_labels, gt_masks, point_coords=None):
        """One iteration on one batch; returns the four loss terms (device scalars, as
        `CrossHead2.loss`) plus `grad_norm` (device scalar, before clipping) and, for a
        `device_targets` trainer, `assign_status` (device int32 scalar; non-zero: the batch's cost
        matrices were refused and the update was skipped).  `feats`: the four backbone feature
        maps -- or, for a trainer built with `backbone=`, the image tensor."""
        head, tape = self.head, self.tape
        self._check_not_repacked()
        if self.swin_stages:                   # the tape runs the whole backbone from the image
            keep = self._drop_path_keep(feats.shape[0]) if self.drop_path else None
            feats = [c.permute(0, 3, 1, 2) for c in self.bb_tape.forward(feats, keep)]
        elif self.backbone is not None:
            feats = [f.clone(memory_format=torch.preserve_format) for f in self.backbone(feats)]
            if self.swin:                      # the taped last stage's C5 feeds the head and loss
                x4 = self.bb_tape.stage_input()
                keep = self._drop_path_keep(x4.shape[0]) if self.drop_path else None
                feats[3] = self.bb_tape.forward(x4, keep).permute(0, 3, 1, 2)
        outs = head.forward(feats, img_metas)
        up = {}
        lkw = dict(device_targets=True) if self.device_targets else {}
        drop = self.dropout_descriptor()
        if drop is None:
            losses = head.loss(*outs, gt_rels, None, gt_labels, gt_masks, img_metas,
                               point_coords=point_coords, grads=up, **lkw)
        pl = head._last_plan
        masks = outs[1]
        if drop is not None and self.train_decoder and head.exact_mask_order == "full":
            # (the dense cross-check mode re-computes each layer's mask logits into the plan's
            # output buffer while taping; the loss below must see the final ones)
            masks = dict(masks, mask=masks["mask"].clone())
        if self.train_decoder:
            tape.forward_from_plan(pl, pl.sub_pos, pl.obj_pos, dropout=drop)
        else:
            tape.forward(pl.q, pl.sub_pos, pl.obj_pos, dropout=drop)
        if drop is not None:
            # the loss the reference optimises in train mode: on the DROPPED relation logits (the
            # tape's); everything else of the outputs is the inference kernels'
            cls = dict(outs[0])
            cls["rel"] = tape.t["rel"]
            losses = head.loss(cls, masks, gt_rels, None, gt_labels, gt_masks, img_metas,
                               point_coords=point_coords, grads=up, **lkw)
        if self.pd_tape is not None:
            self.pd_tape.forward(feats)
        self.reducer.start()
        back = tape.backward(g_rel=up["rel"], g_importance=up["importance"], on_ready=self._ready(0))
        if self.pd_tape is not None:           # back[0]: d memory tokens (HeadGrad)
            dfeats, _ = self.pd_tape.backward(back[0], on_ready=self._ready(1))
            if self.swin_stages:               # dfeats: d C5, d C4, d C3
                self.bb_tape.backward(dfeats[2], dfeats[1], dfeats[0], on_ready=self._ready(2))
            elif self.bb_tape is not None and self.swin:   # d C5; C2-C4 come from frozen stages
                self.bb_tape.backward(dfeats[0], on_ready=self._ready(2))
            elif self.bb_tape is not None:     # dfeats: d C5, d C4, d C3
                self.bb_tape.forward(feats[0])
                self.bb_tape.backward(dfeats[2], dfeats[1], dfeats[0], on_ready=self._ready(2))
        self.reducer.finish()
        # (a call whose sizes exceed the device solver's took the host path, which raises itself)
        guard = head._loss.assign_status if self.device_targets and head._loss.last_on_device \
            else None
        if guard is None:          # (callers that replace `apply_gradients` take no argument)
            self.apply_gradients()
        else:
            self.apply_gradients(guard=guard)
        out = dict(losses)
        out["grad_norm"] = self.clip[0]
        if self.device_targets:
            out["assign_status"] = guard[0] if guard is not None else \
                torch.zeros((), dtype=torch.int32, device=self.dev)
        return out
