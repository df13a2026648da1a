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
ONE flat gradient buffer [BaselineHeadGrad | SegPixelDecoderGrad | BackboneGrad] -> global-norm clip
coefficient on the device -> one guarded AdamW launch over the flat parameter buffer that the head's
(and the backbone's) device weights alias -> refresh, in place, of every derived pack the inference
kernels read.  `step` holds no host wait: the two assignment status words (`seg_status()`,
`rel_status()`) are OR-ed on the device into the AdamW launch's guard, so a refused assignment moves
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
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import hip
from .grad import BackboneGrad
from .seg_grad import BaselineHeadGrad, SegPixelDecoderGrad
from .train import TailTrainer

__all__ = ["BaselineTrainer"]

CUSTOM_KEYS = ("backbone", "transformer_decoder", "pixel_decoder", "decoder_input_projs")


class BaselineTrainer:
    # the trainer's default for `BaselineHeadGrad.masked_keysplit_min_keys`: the smallest measured
    # level at and above which pn_mha_bwd_keysplit_masked_f32 beat pn_mha_bwd_f32 in all three
    # repeats for both mask families (tools/baseline_step_probe.py, profiles/baseline_step.json,
    # labnotes R24.4: 0.27 against 0.46 ms at 4 200 keys, 0.74 against 1.73 ms at 16 700, but 0.26
    # against 0.14 ms at 1 050)
    MASKED_KEYSPLIT_MIN_KEYS = 4200

    def __init__(self, head, backbone=None, lr=1e-4, weight_decay=1e-4, betas=(0.9, 0.999),
                 eps=1e-8, max_norm=0.1, lr_mult=None, decay_mult=None, norm_decay_mult=0.0, seed=0,
                 masked_keysplit_min_keys="default"):
        """`lr_mult` / `decay_mult`: {substring of a parameter name: multiplier} (mmcv's
        `paramwise_cfg.custom_keys`; default: the four keys of the module docstring at 0.1); a
        backbone's parameters appear as "backbone.<name>".  `masked_keysplit_min_keys`: the head
        tape's switch (None: `pn_mha_bwd_f32` for all nine masked cross-attentions); the default
        is the measured `MASKED_KEYSPLIT_MIN_KEYS`."""
        from .swin import SwinTransformerHip
        if not hasattr(head, "_relation_stage") or not hasattr(head, "full_losses"):
            raise NotImplementedError("BaselineTrainer trains a CrossHeadBaseline (%s: TailTrainer)"
                                      % type(head).__name__)
        if isinstance(backbone, SwinTransformerHip):
            raise NotImplementedError("BaselineTrainer trains a ResNet50Hip backbone (stages 2-4); "
                                      "a Swin backbone is out of scope")
        self.head, self.backbone = head, backbone
        self.seed = int(seed)
        if head.w is None:
            head._pack()
        # plans captured so far bake the addresses of the weight tensors that are re-homed below
        # into their hipGraphs: start from fresh plans (the arenas, shape-dependent only, stay)
        from .plans import PlanCache
        head._plans = PlanCache(head._plans.max_plans)
        dev = self.dev = self.device = head.device
        if backbone is not None:
            if backbone.device is None:
                backbone.to(dev)
            if backbone.w is None:
                backbone._pack()
        # ONE flat gradient buffer: [head tape | pixel decoder tape | backbone tape]
        n_head = BaselineHeadGrad.size_of(head)
        n_pd = SegPixelDecoderGrad.size_of(head)
        n_bb = BackboneGrad.size_of(backbone) if backbone is not None else 0
        self.n = n_head + n_pd + n_bb
        self.flat_grad = torch.zeros(self.n, device=dev, dtype=torch.float32)
        self.tape = BaselineHeadGrad(head, flat=self.flat_grad, base=0)
        self.tape.masked_keysplit_min_keys = self.MASKED_KEYSPLIT_MIN_KEYS \
            if isinstance(masked_keysplit_min_keys, str) and masked_keysplit_min_keys == "default" \
            else masked_keysplit_min_keys
        self.pd_tape = SegPixelDecoderGrad(head, flat=self.flat_grad, base=n_head)
        self.bb_tape = BackboneGrad(backbone, flat=self.flat_grad, base=n_head + n_pd) \
            if backbone is not None else None
        self.lr, self.wd, self.betas, self.eps, self.max_norm = lr, weight_decay, betas, eps, max_norm
        # name -> (offset in the shared buffer, shape, numel)
        self.layout = OrderedDict(self.tape.layout)
        for n, (o, shape, k) in self.pd_tape.layout.items():
            self.layout[n] = (o + n_head, shape, k)
        src = {n: head._params[n] for n in self.layout}          # where a parameter's value lives
        if self.bb_tape is not None:
            for n, (o, shape, k) in self.bb_tape.layout.items():
                self.layout["backbone." + n] = (o + n_head + n_pd, shape, k)
                src["backbone." + n] = backbone._params[n]
        self.names = list(self.layout)
        # ---- flat parameters; the head's device weights become views of them ----
        self.flat_p = torch.zeros(self.n, device=dev, dtype=torch.float32)
        self.flat_m = torch.zeros_like(self.flat_p)
        self.flat_v = torch.zeros_like(self.flat_p)
        w = head.w
        self.params = OrderedDict()
        # w[...] holds another layout ([co][(ky * 3 + kx) * 256 + ci]): refreshed, not aliased
        self._repacked = {"pixel_decoder.output_convs.0.conv.weight"}
        for n in self.layout:
            o, shape, k = self.layout[n]
            view = self.flat_p[o:o + k].view(shape)
            view.copy_(src[n].to(dev))
            self.params[n] = view
            if n.startswith("backbone."):
                continue          # the backbone's packed weights are all derived (BatchNorm folded)
            if n not in self._repacked:
                # same bytes as the reference layout (the 1x1 convolutions: [256, C, 1, 1] == [256, C])
                w[n] = view.view(w[n].shape)
        # ---- per-segment multipliers (mmcv paramwise_cfg; module docstring) ----
        lr_mult = dict({k: 0.1 for k in CUSTOM_KEYS} if lr_mult is None else lr_mult)
        decay_mult = dict({k: 0.1 for k in CUSTOM_KEYS} if decay_mult is None else decay_mult)
        offs, lrs, wds = [], [], []
        for n in self.layout:
            offs.append(self.layout[n][0])
            lm, dm = self.multipliers(n, lr_mult, decay_mult, norm_decay_mult)
            lrs.append(lm)
            wds.append(dm)
        offs.append(self.n)
        self.seg_off = torch.tensor(offs, dtype=torch.int64, device=dev)
        self.seg_lr = torch.tensor(lrs, dtype=torch.float32, device=dev)
        self.seg_wd = torch.tensor(wds, dtype=torch.float32, device=dev)
        self.clip = torch.zeros(2, device=dev, dtype=torch.float32)     # [grad norm, coefficient]
        self._scratch = torch.zeros(256, device=dev, dtype=torch.float64)
        self._guard = torch.zeros(1, device=dev, dtype=torch.int32)
        self.steps = 0
        self.last_ready_ends = []
        self._w_dicts = (head.w, backbone.w if backbone is not None else None)
        self._refresh_derived()

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
        if BaselineTrainer.is_norm(name):
            return 1.0, float(norm_decay_mult)
        return 1.0, 1.0

    def _refresh_derived(self):
        """Every weight pack the head's (and the backbone's) INFERENCE kernels read that is a
        function of trained parameters, rewritten in place (captured hipGraphs keep their
        pointers): the two decoders' self-attention [V | Q | K] projections, the batch-repeated
        initial queries and their mask embedding, both position tables (they carry `level_embed` /
        `level_encoding`), the encoder's [value | offsets | weights] projections and bf16-plane
        splits, the FPN branch's 3x3 convolution in its direct and two Winograd forms, and the
        backbone's BatchNorm-folded packs.  Everything else the forward reads (`cls_embed`,
        `rel_cls_embed`, the MLPs, norms, the 1x1 convolutions, `mask_feature`) is a view of the
        flat buffer."""
        head, w, p = self.head, self.head.w, self.params
        for dec, nl, a in (("transformer_decoder", head.num_dec_layers, "attentions.1.attn."),
                           ("relation_decoder", head.num_rel_layers, "attentions.0.attn.")):
            for i in range(nl):                    # self-attention as one [V | Q | K] projection
                pre = "%s.layers.%d.%s" % (dec, i, a)
                W, b = p[pre + "in_proj_weight"], p[pre + "in_proj_bias"]
                w[pre + "vqk.weight"][:256].copy_(W[512:])
                w[pre + "vqk.weight"][256:].copy_(W[:512])
                w[pre + "vqk.bias"][:256].copy_(b[512:])
                w[pre + "vqk.bias"][256:].copy_(b[:512])
        for c in head._consts.values():            # the initial queries repeated over the batch
            if "r0" in c:
                B = c["r0"].shape[0] // p["rel_query_feat.weight"].shape[0]
                c["r0"].view(B, -1, 256).copy_(p["rel_query_feat.weight"].unsqueeze(0).expand(B, -1, -1))
            if "q0" in c:
                BQ = c["q0"].shape[0]
                B = BQ // p["query_feat.weight"].shape[0]
                c["q0"].view(B, -1, 256).copy_(p["query_feat.weight"].unsqueeze(0).expand(B, -1, -1))
                if c.get("me0") is not None:       # ... and their mask embedding
                    tmp = SimpleNamespace(B=B, cls=None, MP=None,
                                          **{n: torch.empty(BQ, 256, device=self.dev)
                                             for n in ("qn", "m1", "m2", "me")})
                    head._head_embed(c["q0"], tmp, False, False)
                    c["me0"].copy_(tmp.me)
        pd = "pixel_decoder."
        for shapes, ent in head._pe.items():
            o = 0
            for l, (h, wd) in enumerate(shapes):
                hip.sine_pe(ent[1][l], p["level_embed.weight"][l], h, wd)       # key positions
                hip.sine_pe(ent[0][o:o + h * wd], p[pd + "level_encoding.weight"][l], h, wd)
                o += h * wd
            ent[3].copy_(hip.pos8(ent[0]))
        for i in range(head.num_enc_layers):
            q, a = pd + "encoder.layers.%d." % i, pd + "encoder.layers.%d.attentions.0." % i
            o = 0
            for n in ("value_proj", "sampling_offsets", "attention_weights"):
                r = p[a + n + ".weight"].shape[0]
                w[a + "voa.weight"][o:o + r].copy_(p[a + n + ".weight"])
                w[a + "voa.bias"][o:o + r].copy_(p[a + n + ".bias"])
                o += r
            for k in (a + "voa.weight", a + "output_proj.weight", q + "ffns.0.layers.0.0.weight",
                      q + "ffns.0.layers.1.weight"):
                hip.s3_split(w[k], w[k + ".s3"])              # the bf16-pipe GEMMs' operands
        c3 = pd + "output_convs.0.conv."
        cw = p[c3 + "weight"]
        w[c3 + "winograd"].copy_(hip.winograd_weights(cw))
        w[c3 + "winograd4"].copy_(hip.winograd43_weights(cw))
        w[c3 + "weight"].copy_(cw.permute(0, 2, 3, 1).reshape(256, -1))
        if self.bb_tape is not None:
            TailTrainer._refresh_backbone(self)

    def set_epoch(self, epoch, steps=(40,), gamma=0.1):
        """The config's learning-rate schedule (`lr_config = dict(policy="step", step=40)`, by
        epoch; mmcv's default gamma): sets `self.lr` for 0-based `epoch`."""
        if not hasattr(self, "base_lr"):
            self.base_lr = self.lr
        self.lr = self.base_lr * gamma ** sum(1 for s in steps if epoch >= s)
        return self.lr

    def write_back(self):
        """Copy the trained values into the head's (and the backbone's) state dict."""
        head = self.head
        for n, v in self.params.items():
            dst = self.backbone._params[n[len("backbone."):]] if n.startswith("backbone.") \
                else head._params[n]
            dst.copy_(v.to(dst.device))
        head._packed_version = head._weights_version()     # the packed device weights ARE these values
        if self.backbone is not None and hasattr(self.backbone, "_weights_version"):
            self.backbone._packed_version = self.backbone._weights_version()

    # ------------------------------------------------------------------
    @torch.no_grad()
    @hip.on_device
    def step(self, feats, img_metas, gt_rels, gt_labels, gt_masks, num_total_masks=None):
        """One iteration on one batch.  `feats`: the four backbone feature maps -- or, for a
        trainer built with `backbone=`, the image tensor.  `gt_masks` at half the batch tensor's
        size (`PSGTr._prepare_gt_masks`).  Returns the 30 loss terms of `full_losses` plus
        `grad_norm` (before clipping) and `assign_status` (int32; non-zero: an assignment was
        refused and the update was skipped), all device scalars."""
        head, tape = self.head, self.tape
        if head.w is not self._w_dicts[0] or (self.backbone is not None
                                              and self.backbone.w is not self._w_dicts[1]):
            raise RuntimeError("the head (or backbone) re-packed its weights since this "
                               "BaselineTrainer was built (load_state_dict, parameter update, "
                               ".to()): build a new one")
        if self.backbone is not None:
            feats = [f.clone(memory_format=torch.preserve_format) for f in self.backbone(feats)]
        keep = head.return_all_layers
        head.return_all_layers = True
        try:
            cls, masks = head.forward(feats, img_metas)
        finally:
            head.return_all_layers = keep
        pl = head._last_plan
        up = {}
        losses = head.full_losses(cls, masks, gt_rels, None, gt_labels, gt_masks, img_metas,
                                  grads=up, seed=self.seed, step=self.steps,
                                  num_total_masks=num_total_masks)
        nh, npd = tape.flat_numel, self.pd_tape.flat_numel
        ends = self.last_ready_ends = []
        tape.forward_from_plan(pl)
        dmem, dMF, _ = tape.backward(up, counts=head._seg_loss.last["counts"],
                                     on_ready=lambda e: ends.append(min(e, nh)))
        self.pd_tape.forward(feats)
        dfeats, _ = self.pd_tape.backward(dmem, dMF, on_ready=lambda e: ends.append(nh + min(e, npd)))
        if self.bb_tape is not None:               # dfeats: d C5, d C4, d C3 (, d C2: layer1 is frozen)
            self.bb_tape.forward(feats[0])
            self.bb_tape.backward(dfeats[2], dfeats[1], dfeats[0],
                                  on_ready=lambda e: ends.append(nh + npd + e))
        torch.bitwise_or(head.seg_status().view(1), head.rel_status().view(1), out=self._guard)
        self.apply_gradients(guard=self._guard)
        out = dict(losses)
        out["grad_norm"] = self.clip[0]
        out["assign_status"] = self._guard[0]
        return out

    @torch.no_grad()
    @hip.on_device
    def apply_gradients(self, guard=None):
        """Clip (global L2 norm over the whole flat gradient) + AdamW on `flat_grad`, then the
        refresh of the derived packs.  `guard`: a device int32 word; non-zero skips the update on
        the device (`steps` advances all the same)."""
        g = self.flat_grad
        hip.grad_norm_clip(g, self.clip, self._scratch, pre=1.0, max_norm=self.max_norm)
        self.steps += 1
        hip.adamw(self.flat_p, g, self.flat_m, self.flat_v, self.seg_off, self.seg_lr, self.seg_wd,
                  self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self.steps,
                  clip=self.clip, pre=1.0, guard=guard)
        self._refresh_derived()
