"""CrossHead2 on MI355X: the Pair-Net head behind the reference's own interface.

Mirrors pairnet/models/relation_heads/pairnet_head.py (`CrossHead2`): constructor
keywords (:24-55), `forward(feats, img_metas)` (:260-417), `forward_head` (:216-258),
`get_bboxes` (:760-786), `simple_test_bboxes` (:926-930) and the state-dict key names
(SURVEY.md 8a N7), so `configs/mask2former/pairnet.py` and a reference checkpoint
drop in.  All arithmetic runs in the hand-written gfx950 kernels of
libpairnet_hip.so through `hip.py`; torch supplies device buffers, views, memcpys
and the stream.  There is no CPU path: every entry raises without the library/GPU.

Device data layout (fp32, batch-first, channel-last):
  tokens X        [B, N0+N1+N2, 256]   encoder tokens, levels low->high resolution
  mask feature    [B, H2*W2, 256]      pixel-major, so mask logits are an NT GEMM
  queries         [B*Q, 256]
The reference's seq-first (Q,B,C) / NCHW layouts exist only at the API boundary.
"""
import math
from collections import OrderedDict

import torch

from . import hip
from . import plans
from .plans import Arena, PlanCache, measure_bytes
from .config import ConfigDict

INSTANCE_OFFSET = 1000


def _decoder_param_shapes(prefix, num_layers, ffn_dim, out):
    for i in range(num_layers):
        p = "%s.layers.%d." % (prefix, i)
        for a in (0, 1):
            out[p + "attentions.%d.attn.in_proj_weight" % a] = (768, 256)
            out[p + "attentions.%d.attn.in_proj_bias" % a] = (768,)
            out[p + "attentions.%d.attn.out_proj.weight" % a] = (256, 256)
            out[p + "attentions.%d.attn.out_proj.bias" % a] = (256,)
        out[p + "ffns.0.layers.0.0.weight"] = (ffn_dim, 256)
        out[p + "ffns.0.layers.0.0.bias"] = (ffn_dim,)
        out[p + "ffns.0.layers.1.weight"] = (256, ffn_dim)
        out[p + "ffns.0.layers.1.bias"] = (256,)
        for n in range(3):
            out[p + "norms.%d.weight" % n] = (256,)
            out[p + "norms.%d.bias" % n] = (256,)
    out[prefix + ".post_norm.weight"] = (256,)
    out[prefix + ".post_norm.bias"] = (256,)


def _drop_rates(cfg, prefix=""):
    """{dotted config key: rate} of every non-zero dropout setting below `cfg` (mmcv's spellings:
    `ffn_drop`, `attn_drop`, `proj_drop`, MultiScaleDeformableAttention's `dropout`, and a
    `dropout_layer=dict(type=..., drop_prob=)`)."""
    out = OrderedDict()
    items = cfg.items() if isinstance(cfg, dict) else enumerate(cfg)
    for k, v in items:
        key = "%s%s" % (prefix, k)
        if k == "dropout_layer" and isinstance(v, dict):
            v = v.get("drop_prob", 0.0)
        if k in ("ffn_drop", "attn_drop", "proj_drop", "dropout", "dropout_layer"):
            if isinstance(v, (int, float)) and float(v) != 0.0:
                out[key] = float(v)
        elif isinstance(v, (dict, list, tuple)):
            out.update(_drop_rates(v, key + "."))
    return out


class CrossHead2:
    """Drop-in for the reference's `CrossHead2` (inference half)."""

    # operation order of the relation decoder's layers this head is built for
    RELATION_ORDER = ("cross_attn", "norm", "self_attn", "norm", "ffn", "norm")
    POST_ENTRIES = 8     # post-processing buffer sets kept per plan / for foreign inputs

    def __init__(self, num_classes, in_channels, num_relations, num_obj_query=100,
                 num_rel_query=100, mapper="conv_tiny", use_mask=True, pixel_decoder=None,
                 transformer_decoder=None, feat_channels=256, out_channels=256,
                 num_transformer_feat_level=3, embed_dims=256, relation_decoder=None,
                 enforce_decoder_input_project=False, n_heads=8,
                 positional_encoding=dict(type="SinePositionalEncoding", num_feats=128,
                                          normalize=True),
                 rel_cls_loss=None, subobj_cls_loss=None, importance_match_loss=None,
                 loss_cls=None, loss_mask=None, loss_dice=None, train_cfg=None,
                 test_cfg=dict(max_per_img=100), init_cfg=None, **kwargs):
        pixel_decoder = ConfigDict(pixel_decoder)
        transformer_decoder = ConfigDict(transformer_decoder)
        relation_decoder = ConfigDict(relation_decoder)
        if mapper != "conv_tiny":
            raise NotImplementedError("only mapper='conv_tiny' (configs/mask2former/pairnet.py:26)")
        # train_cfg (mmdet passes the model-level one to the head): kept for `loss()` -- the
        # VALUES of the reference's loss and their gradients w.r.t. the logits (losses.py); the
        # backward through the network and the optimizer step live in grad.py / train.py
        self._loss_cfg = dict(train_cfg=train_cfg, rel_cls_loss=rel_cls_loss,
                              subobj_cls_loss=subobj_cls_loss,
                              importance_match_loss=importance_match_loss)
        self._loss = None
        # the same checks the reference makes (pairnet_head.py:72-87)
        assert "num_feats" in positional_encoding
        assert positional_encoding["num_feats"] * 2 == embed_dims
        enc_attn = pixel_decoder.encoder.transformerlayers.attn_cfgs
        assert enc_attn.num_levels == num_transformer_feat_level
        if (feat_channels, out_channels, embed_dims, n_heads) != (256, 256, 256, 8):
            raise NotImplementedError("kernels are built for 256 channels, 8 heads")
        if transformer_decoder.transformerlayers.attn_cfgs.num_heads != 8 or enforce_decoder_input_project:
            raise NotImplementedError("8-head decoder without input projection only")
        if (enc_attn.num_heads, enc_attn.num_points, enc_attn.embed_dims) != (8, 4, 256):
            raise NotImplementedError("MSDeformAttn kernel: 8 heads, 4 points")
        for dec, want in ((transformer_decoder, CrossHead2.RELATION_ORDER),
                          (relation_decoder, self.RELATION_ORDER)):
            got = tuple(dec.transformerlayers.get("operation_order", want))
            if got != want:
                raise NotImplementedError("operation_order %s (built for %s)" % (got, want))
        self.num_classes = num_classes
        self.num_relations = num_relations
        self.num_obj_query = self.num_queries = num_obj_query
        self.num_rel_query = num_rel_query
        self.use_mask = use_mask
        self.n_heads = self.num_heads = n_heads
        self.embed_dims = embed_dims
        self.in_channels = list(in_channels)
        self.num_transformer_feat_level = num_transformer_feat_level
        self.num_enc_layers = pixel_decoder.encoder.num_layers
        self.enc_ffn = pixel_decoder.encoder.transformerlayers.ffn_cfgs.feedforward_channels
        self.gn_groups = pixel_decoder.norm_cfg.num_groups
        self.num_dec_layers = transformer_decoder.num_layers
        self.dec_ffn = transformer_decoder.transformerlayers.ffn_cfgs.feedforward_channels
        self.num_rel_layers = relation_decoder.num_layers
        self.rel_ffn = relation_decoder.transformerlayers.ffn_cfgs.feedforward_channels
        # the one non-zero dropout rate of the reference's config (pairnet.py:126): the training
        # step honours it on request (train.py `dropout=`); inference never drops.  Every OTHER
        # configured rate is recorded by its key so that the trainer can refuse what it cannot do.
        self.rel_ffn_drop = float(relation_decoder.transformerlayers.ffn_cfgs.get("ffn_drop", 0.0))
        self.other_drop_rates = _drop_rates(dict(pixel_decoder=pixel_decoder,
                                                 transformer_decoder=transformer_decoder,
                                                 relation_decoder=relation_decoder))
        self.other_drop_rates.pop("relation_decoder.transformerlayers.ffn_cfgs.ffn_drop", None)
        self.test_cfg, self.train_cfg = test_cfg, train_cfg
        assert len(self.in_channels) == 4 and num_transformer_feat_level == 3
        assert num_obj_query <= 256 and num_rel_query <= 128
        self._params = OrderedDict(
            (k, torch.zeros(s)) for k, s in self.param_shapes().items())
        self.device = None
        self.w = None
        self._plans = PlanCache()
        self._arenas, self._post_arenas, self._consts, self._pe = {}, {}, {}, OrderedDict()
        self._dummies = {}
        self._post = OrderedDict()
        self._pan_jobs = []
        # stage graphs are captured once a (shape, slot) has been run this many times eagerly
        # (with the per-slot arenas an eager first sight costs no allocation and no host
        # synchronisation, and the pipelined eager rate is within 0.5 % of the replayed one:
        # a shape that shows up once is never captured)
        self.graph_after = 1
        # Attention masks (see _attn_mask).  True (default since round 3): the reference's
        # operation order -- full-size mask logits -> bilinear resize -> threshold -- evaluated
        # at the 4 logits per key the resize reads; "full": the same, densely (bit-identical,
        # the cross-check); False: opt-in shortcut, logits against the mask feature resampled
        # once per level (+2.5 % images/s, a different fp32 rounding of the same logits)
        self.exact_mask_order = True
        # 3x3 FPN convolution (every mode is fp32 arithmetic on the fp32 MFMA): "winograd4" =
        # F(4x4,3x3), 4x fewer multiplications, ~1.6e-5 relative to the direct form (default:
        # the end-to-end errors against the reference are the same to three digits for all
        # three modes, tests/test_head_gpu.py::test_e2e_full_800x1333_...); "winograd" =
        # F(2x2,3x3), 2.25x fewer, ~2e-6 (needs even sides of the 1/4-resolution map, else
        # "direct" is used); "direct" = implicit GEMM (bitwise an fmaf chain)
        self.conv_algo = "winograd4"
        # replay each stage as one hipGraph (no per-launch host cost) after a warm-up call
        self.use_graphs = False
        # persistent-GEMM workgroup slots stage A leaves free for concurrent streams' kernels
        # (a per-call hint, hip.reserve_slots; PipelinedHead sets it for its own schedule)
        self.grid_reserve = 0
        self.fuse_ppn_front = True      # normalise + cosine matrix + first Matrix Learner layer in one launch
        # a layer's attention-mask bits (reference operation order) as one launch: stencil
        # logits, blend, threshold and pack in the GEMM's epilogue (pn_mask_stencil_gemm_f32;
        # bit-identical to the GEMM -> pn_mask_pack_stencil pair, which False restores)
        self.fuse_mask_pack = True
        # ... and that launch gathers its stencil rows from the mask feature itself
        # (pn_mask_stencil_gather_gemm_f32): stage A no longer copies them into pl.MFs, three
        # launches and 90 MB of writes per 800 x 1333 image; bit-identical, False restores the copies
        self.gather_mask_stencil = True
        # the encoder layers' FFN (Linear-ReLU-Linear + identity + norms.1) as ONE launch on the
        # bf16x3 path (pn_gemm_s3_ffn_f32): the 1024 hidden values of a row go from FFN-1's
        # registers through LDS into FFN-2's MFMAs instead of through pl.HS, 270 MB of traffic per
        # layer at 800 x 1333; bit-identical, 0 restores the two launches (labnotes R34)
        self.fuse_encoder_ffn = 1
        # the encoder layers' output_proj + identity + norms.0 reads the sampling kernel's fp32 rows
        # itself (pn_gemm_s3_rows_ln_f32: its waves split the rows on their way into LDS) instead of
        # a split pass pl.S -> pl.SS in front of it, one launch and 56 MB of traffic per layer at
        # 800 x 1333; bit-identical, 0 restores the split pass (labnotes R35)
        self.enc_proj_reads_rows = 1
        # lateral GroupNorm and the top-down upsample-add as one pass over the stride-4 map
        # (pn_groupnorm_upadd_nhwc_f32) instead of two, bit-identical.  Off by default: 78 against
        # 90 us stand-alone, but no difference in the pipelined step beyond its run-to-run spread
        # (labnotes R7.3)
        self.fuse_lateral_upadd = False
        # encoder sites whose Linear + identity + LayerNorm run as one row-owning launch
        # (pn_linear_res_ln_f32): "proj" = output_proj -> norms.0, "ffn" = FFN-2 -> norms.1;
        # () = the GEMM -> LayerNorm pairs of rounds 1-3 (bit-identical either way)
        self.enc_fused_ln = ("proj", "ffn")
        # the pixel decoder's three 1x1 input convolutions as one grouped GEMM launch
        # (channels_last features only) instead of three split-K launches.  Off: measured in
        # round 4, three alternating 300-step runs: grouped 207.7 / 208.3 / 207.9 images/s,
        # split 209.9 / 209.4 / 209.8 -- the grouped kernel has no K split, and the 68 deep-K
        # tiles of the C5 convolution (64 chunks each) become its tail
        self.group_input_convs = False
        # arithmetic of the encoder's GEMMs (value / offsets / logits projection, output_proj,
        # FFN: 192 of the head's 364 GFLOP at 800x1333).  "bf16x3" (default, round 6): fp32
        # operands kept as three exact bf16 planes by the kernels that produce them, six bf16 MFMA
        # products, fp32 accumulation (csrc/gemm_s3.hip: error against fp64 at or below the fp32
        # MFMA's); "fp32": the exact-fp32 MFMA kernels of rounds 1-5 (pn_gemm_f32,
        # pn_linear_res_ln_f32).  Everything else is fp32 MFMA either way.
        self.gemm_arithmetic = "bf16x3"
        # bf16x3: the sampling kernel can write output_proj's A operand pre-split (True) instead of
        # fp32 rows + a split pass (False): the same values either way (tested bit for bit), but
        # its scattered 16-byte stores cost the L1-bound kernel 8 us per layer where the split
        # pass costs 12, and under the pipeline the step is the same (221.1 vs 219.7 images/s,
        # labnotes R6.5): off
        self.msda_s3_out = False
        # the subject / object result masks of the head's own outputs straight from the mask
        # logits (pn_pair_masks_u8): stage B no longer gathers MP[sub_pos] / MP[obj_pos] into
        # sub_seg / obj_seg (107 MB moved per 800 x 1333 image) and get_bboxes resamples every
        # referenced object once instead of every slot; bit-identical.  forward() still returns
        # the gathered logits (it issues the two gathers itself); False restores the launches
        # of rounds 1-11
        self.fused_pair_masks = True
        self.init_weights()

    # ------------------------------------------------------------------ params
    def param_shapes(self):
        """Reference state-dict names -> shapes."""
        s = OrderedDict()
        Q, R = self.num_obj_query, self.num_rel_query
        _decoder_param_shapes("relation_decoder", self.num_rel_layers, self.rel_ffn, s)
        s["rel_query_embed.weight"] = (R, 256)
        s["rel_query_embed2.weight"] = (2 * R, 256)
        s["rel_query_embed3.weight"] = (2 * R, 256)  # dead weight (Appendix B)
        s["rel_query_feat.weight"] = (R, 256)
        for i, (ci, co) in enumerate(((1, 64), (64, 64), (64, 1))):
            s["update_importance.conv_layers.%d.0.weight" % i] = (co, ci, 7, 7)
            s["update_importance.conv_layers.%d.0.bias" % i] = (co,)
        pd = "pixel_decoder."
        for i in range(3):
            cin = self.in_channels[3 - i]
            s[pd + "input_convs.%d.conv.weight" % i] = (256, cin, 1, 1)
            s[pd + "input_convs.%d.conv.bias" % i] = (256,)
            s[pd + "input_convs.%d.gn.weight" % i] = (256,)
            s[pd + "input_convs.%d.gn.bias" % i] = (256,)
        for i in range(self.num_enc_layers):
            p = pd + "encoder.layers.%d." % i
            for name, n in (("sampling_offsets", 192), ("attention_weights", 96),
                            ("value_proj", 256), ("output_proj", 256)):
                s[p + "attentions.0.%s.weight" % name] = (n, 256)
                s[p + "attentions.0.%s.bias" % name] = (n,)
            s[p + "ffns.0.layers.0.0.weight"] = (self.enc_ffn, 256)
            s[p + "ffns.0.layers.0.0.bias"] = (self.enc_ffn,)
            s[p + "ffns.0.layers.1.weight"] = (256, self.enc_ffn)
            s[p + "ffns.0.layers.1.bias"] = (256,)
            for n in range(2):
                s[p + "norms.%d.weight" % n] = (256,)
                s[p + "norms.%d.bias" % n] = (256,)
        s[pd + "level_encoding.weight"] = (3, 256)
        s[pd + "lateral_convs.0.conv.weight"] = (256, self.in_channels[0], 1, 1)
        s[pd + "lateral_convs.0.gn.weight"] = (256,)
        s[pd + "lateral_convs.0.gn.bias"] = (256,)
        s[pd + "output_convs.0.conv.weight"] = (256, 256, 3, 3)
        s[pd + "output_convs.0.gn.weight"] = (256,)
        s[pd + "output_convs.0.gn.bias"] = (256,)
        s[pd + "mask_feature.weight"] = (256, 256, 1, 1)
        s[pd + "mask_feature.bias"] = (256,)
        _decoder_param_shapes("transformer_decoder", self.num_dec_layers, self.dec_ffn, s)
        s["query_embed.weight"] = (Q, 256)
        s["query_feat.weight"] = (Q, 256)
        s["level_embed.weight"] = (3, 256)
        s["cls_embed.weight"] = (self.num_classes + 1, 256)
        s["cls_embed.bias"] = (self.num_classes + 1,)
        for mlp in ("mask_embed", "sub_query_update", "obj_query_update"):
            for j in (0, 2, 4):
                s["%s.%d.weight" % (mlp, j)] = (256, 256)
                s["%s.%d.bias" % (mlp, j)] = (256,)
        s["rel_cls_embed.weight"] = (self.num_relations, 256)
        s["rel_cls_embed.bias"] = (self.num_relations,)
        return s

    def init_weights(self, seed=0):
        """Random init with the distributions the reference ends up with
        (torch layer defaults, then pairnet_head.py:177-193 / mmdet pixel-decoder
        init): not the reference's RNG stream, the same families."""
        g = torch.Generator().manual_seed(seed)
        U = lambda shape, b: (torch.rand(shape, generator=g) * 2 - 1) * b
        N = lambda shape, std: torch.randn(shape, generator=g) * std
        for k, p in self._params.items():
            shape = tuple(p.shape)
            leaf = k.rsplit(".", 1)[-1]
            in_decoder = k.startswith(("transformer_decoder.", "relation_decoder.",
                                       "pixel_decoder.encoder."))
            if ".norms." in k or ".gn." in k or "post_norm" in k:
                v = torch.ones(shape) if leaf == "weight" else torch.zeros(shape)
            elif len(shape) == 1:
                wshape = self._params[k[:-len("bias")] + "weight"].shape
                fan_in = 1
                for d in wshape[1:]:
                    fan_in *= d
                v = torch.zeros(shape) if ("in_proj" in k or "out_proj" in k) \
                    else U(shape, 1.0 / math.sqrt(fan_in))
            elif in_decoder:  # xavier_normal_ on every matrix
                fan_out, fan_in = shape[0], shape[1]
                v = N(shape, math.sqrt(2.0 / (fan_in + fan_out)))
            elif k.endswith(("query_embed.weight", "query_feat.weight", "query_embed2.weight",
                             "query_embed3.weight", "level_embed.weight",
                             "level_encoding.weight")):
                v = N(shape, 1.0)
            else:  # Linear / Conv2d default: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
                fan_in = 1
                for d in shape[1:]:
                    fan_in *= d
                v = U(shape, 1.0 / math.sqrt(fan_in))
            p.copy_(v)
        # MultiScaleDeformableAttention.init_weights: zero weights, directional
        # grid bias for the offsets, uniform attention
        thetas = torch.arange(8, dtype=torch.float32) * (2.0 * math.pi / 8)
        grid = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid = (grid / grid.abs().max(-1, keepdim=True)[0]).view(8, 1, 1, 2).repeat(1, 3, 4, 1)
        for i in range(4):
            grid[:, :, i, :] *= i + 1
        for i in range(self.num_enc_layers):
            p = "pixel_decoder.encoder.layers.%d.attentions.0." % i
            self._params[p + "sampling_offsets.weight"].zero_()
            self._params[p + "sampling_offsets.bias"].copy_(grid.reshape(-1))
            self._params[p + "attention_weights.weight"].zero_()
            self._params[p + "attention_weights.bias"].zero_()
            for n in ("value_proj", "output_proj"):
                self._params[p + n + ".weight"].copy_(U((256, 256), math.sqrt(6.0 / 512)))
                self._params[p + n + ".bias"].zero_()
        self._drop_weight_state()

    def _drop_weight_state(self):
        """Everything derived from the parameters: packed weights, the per-batch constants
        (initial queries and their mask embedding), position tables with the level embeddings
        folded in, and the plans' hipGraphs (a captured graph bakes the pointers in).  The
        arenas stay: they depend on shapes only."""
        self.w = None
        self._plans = PlanCache(self._plans.max_plans)
        self._consts, self._pe = {}, OrderedDict()

    def _weights_version(self):
        """Changes whenever a parameter tensor is written in place (torch's per-tensor version
        counters): `parameters()` hands out the live tensors, and an optimizer step or a manual
        `p.copy_()` must not leave packed weights, constants and captured graphs stale."""
        return sum(p._version for p in self._params.values())

    def parameters(self):
        """The live (host, fp32) parameter tensors; in-place updates are picked up by the next
        forward (the packed device copies and everything derived from them are rebuilt)."""
        return list(self._params.values())

    def state_dict(self):
        return OrderedDict((k, v.clone()) for k, v in self._params.items())

    def load_state_dict(self, sd, strict=True):
        missing = [k for k in self._params if k not in sd]
        unexpected = [k for k in sd if k not in self._params]
        if strict and (missing or unexpected):
            raise RuntimeError("state_dict mismatch: missing %s unexpected %s"
                               % (missing[:5], unexpected[:5]))
        for k, p in self._params.items():
            if k in sd:
                if tuple(sd[k].shape) != tuple(p.shape):
                    raise RuntimeError("shape mismatch for %s: %s vs %s"
                                       % (k, tuple(sd[k].shape), tuple(p.shape)))
                p.copy_(sd[k].detach().to(torch.float32).cpu())
        self._drop_weight_state()
        return missing, unexpected

    def eval(self):
        return self

    def to(self, device):
        self.device = torch.device(device)
        self._drop_weight_state()
        self._arenas, self._post_arenas = {}, {}
        self._post.clear()
        return self

    def cuda(self, index=0):
        return self.to("cuda:%d" % index)

    # -------------------------------------------------------------- packing
    def _pack(self):
        """Upload parameters in the layouts the kernels read."""
        if self.device is None or self.device.type != "cuda":
            raise RuntimeError("CrossHead2 runs on an MI355X only: call .to('cuda:0'); "
                               "there is no CPU path")
        hip.lib()
        dev = self.device
        w = {k: v.to(dev).contiguous() for k, v in self._params.items()}
        pd = "pixel_decoder."
        for i in range(3):
            k = pd + "input_convs.%d.conv.weight" % i
            w[k] = w[k].reshape(256, -1)
        w[pd + "lateral_convs.0.conv.weight"] = w[pd + "lateral_convs.0.conv.weight"].reshape(256, -1)
        w[pd + "mask_feature.weight"] = w[pd + "mask_feature.weight"].reshape(256, 256)
        # 3x3 conv: Winograd F(2x2,3x3) weights U [16][co][ci] (default algorithm), and
        # [co][ci][ky][kx] -> [co][(ky*3+kx)*256 + ci] for the direct implicit GEMM
        w[pd + "output_convs.0.conv.winograd"] = \
            hip.winograd_weights(w[pd + "output_convs.0.conv.weight"])
        w[pd + "output_convs.0.conv.winograd4"] = \
            hip.winograd43_weights(w[pd + "output_convs.0.conv.weight"])
        w[pd + "output_convs.0.conv.weight"] = \
            w[pd + "output_convs.0.conv.weight"].permute(0, 2, 3, 1).reshape(256, -1).contiguous()
        for i in range(self.num_enc_layers):
            p = pd + "encoder.layers.%d.attentions.0." % i
            # one GEMM per layer: columns [value_proj 256 | sampling_offsets 192 |
            # attention_weights 96]; the positional add feeds only columns >= 256
            w[p + "voa.weight"] = torch.cat([w[p + "value_proj.weight"],
                                             w[p + "sampling_offsets.weight"],
                                             w[p + "attention_weights.weight"]], 0).contiguous()
            w[p + "voa.bias"] = torch.cat([w[p + "value_proj.bias"],
                                           w[p + "sampling_offsets.bias"],
                                           w[p + "attention_weights.bias"]], 0).contiguous()
        # the encoder's weights as S3 operands (three bf16 planes; exact), split once
        for i in range(self.num_enc_layers):
            p = pd + "encoder.layers.%d." % i
            for k in (p + "attentions.0.voa.weight", p + "attentions.0.output_proj.weight",
                      p + "ffns.0.layers.0.0.weight", p + "ffns.0.layers.1.weight"):
                s3 = torch.empty(hip.s3_floats(*w[k].shape), device=dev, dtype=torch.float32)
                hip.s3_split(w[k], s3)
                w[k + ".s3"] = s3
        self._pack_relation(w)
        self.w = w
        self._packed_version = self._weights_version()

    @staticmethod
    def _pack_vqk(w, attn_prefix):
        """Self-attention as one [V | Q | K] projection (the positional add feeds only
        the Q and K columns)."""
        W, b = w[attn_prefix + "in_proj_weight"], w[attn_prefix + "in_proj_bias"]
        w[attn_prefix + "vqk.weight"] = torch.cat([W[512:], W[:512]], 0).contiguous()
        w[attn_prefix + "vqk.bias"] = torch.cat([b[512:], b[:512]], 0).contiguous()

    def _pack_relation(self, w):
        for dec, n in (("transformer_decoder", self.num_dec_layers),
                       ("relation_decoder", self.num_rel_layers)):
            for i in range(n):
                self._pack_vqk(w, "%s.layers.%d.attentions.1.attn." % (dec, i))
        # relation cross-attention keys/values: one [V | K] projection
        for i in range(self.num_rel_layers):
            a = "relation_decoder.layers.%d.attentions.0.attn." % i
            W, b = w[a + "in_proj_weight"], w[a + "in_proj_bias"]
            w[a + "vk.weight"] = torch.cat([W[512:], W[256:512]], 0).contiguous()
            w[a + "vk.bias"] = torch.cat([b[512:], b[256:512]], 0).contiguous()
        ml = "update_importance.conv_layers."
        w[ml + "0.0.weight"] = w[ml + "0.0.weight"].reshape(64, 49).contiguous()
        w[ml + "1.0.weight"] = w[ml + "1.0.weight"].permute(0, 2, 3, 1).reshape(64, -1).contiguous()
        w[ml + "2.0.weight"] = w[ml + "2.0.weight"].reshape(64, 49).t().contiguous()

    class _Plan:
        """Views of one pipeline slot's arena for one (batch, feature shapes) + the hipGraphs
        captured on them."""

        def busy_events(self):
            """Events behind everything queued so far on the streams this plan ran on (the
            plan cache parks an evicted plan until they have fired)."""
            out = []
            for st in getattr(self, "streams", {}).values():
                ev = torch.cuda.Event()
                ev.record(st)
                out.append(ev)
            return out

    STAGE_A_GRAPHS = 4   # stage-A graphs kept per plan (one per set of caller feature buffers)
    PE_SHAPES = 24       # position tables kept (LRU), shared by the slots: ~44 MB per full-size shape
    POST_VIEWS = 8       # post-processing view sets / get_bboxes graphs kept per plan

    def _arena(self, slot):
        """The flat buffer of pipeline slot `slot` (plans.py): every plan of the slot is a
        set of views of it.  When it grows, the slot's plans are dropped."""
        a = self._arenas.get(slot)
        if a is None:
            a = self._arenas[slot] = Arena(self.device, on_grow=lambda a, s=slot: self._plans.drop(
                lambda k: k[3] == s))
        return a

    def _post_arena(self, slot):
        """The slot's second arena, for the post-processing buffers (sized by the ORIGINAL
        image size, which is independent of the padded tensor shape).  When it grows, the
        slot's plans keep their views of the main arena and forget their post-processing
        views and `get_bboxes` graphs."""
        a = self._post_arenas.get(slot)
        if a is None:
            def on_grow(arena, s=slot):
                for k, pl in self._plans.items():
                    if k[3] == s:
                        pl.post_views, pl.graph_c = OrderedDict(), PlanCache(self.POST_VIEWS)
            a = self._post_arenas[slot] = Arena(self.device, on_grow=on_grow)
        return a

    def _const(self, B):
        """Weight-derived, shape-independent constants of batch size B, shared by every plan:
        the initial object / relation queries repeated over the batch (`query_feat`,
        `rel_query_feat`: the first layer reads them in place) and -- filled by `_plan` --
        `me0`, the mask embedding of the initial queries."""
        c = self._consts.get(B)
        if c is None:
            w = self.w
            rep = lambda t: t.unsqueeze(0).expand(B, *t.shape).reshape(B * t.shape[0], 256).contiguous()
            c = self._consts[B] = dict(me0=None)
            for name, key in (("q0", "query_feat.weight"), ("r0", "rel_query_feat.weight")):
                if key in w:        # (the box trunk has no learned object queries)
                    c[name] = rep(w[key])
        return c

    def _position_tables(self, shapes):
        """Sine position tables (+ level embeddings) of a feature pyramid: read-only, the
        same for every slot and batch size -> one copy per shape, LRU-bounded.  Returns
        (enc_pos [SN,256], [dec_kpos_l], event behind the kernels that fill them)."""
        key = tuple(shapes)
        ent = self._pe.get(key)
        if ent is not None:
            self._pe.move_to_end(key)
            return ent
        w, dev = self.w, self.device
        N = [h * wd for h, wd in shapes]
        enc_pos = torch.empty(sum(N), 256, device=dev, dtype=torch.float32)
        dec_kpos, o = [], 0
        for l, (h, wd) in enumerate(shapes):
            hip.sine_pe(enc_pos[o:o + N[l]], w["pixel_decoder.level_encoding.weight"][l], h, wd)
            kp = torch.empty(N[l], 256, device=dev, dtype=torch.float32)
            hip.sine_pe(kp, w["level_embed.weight"][l], h, wd)
            dec_kpos.append(kp)
            o += N[l]
        # the encoder table once more in the order gemm_s3's `out + pos` epilogue reads
        enc_pos8 = hip.pos8(enc_pos)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        ent = self._pe[key] = (enc_pos, dec_kpos, ev, enc_pos8)
        while len(self._pe) > self.PE_SHAPES:
            # the plans of a shape whose tables go are dropped with them (their graphs bake
            # the tables' addresses in; parked until idle, plans.py): device memory per shape
            # is these tables and nothing else, for at most PE_SHAPES shapes
            old, _ = self._pe.popitem(last=False)
            self._plans.drop(lambda k: k[1] == old)
        return ent

    @staticmethod
    def _plan_dims(B, shapes, hw2):
        return (B, hw2[0], hw2[1]) + tuple(v for hw in shapes for v in hw)

    def _layout_for(self, dims, nhwc=False):
        B, hw2 = dims[0], (dims[1], dims[2])
        shapes = [(dims[3 + 2 * l], dims[4 + 2 * l]) for l in range(3)]

        def layout(E):
            pl = CrossHead2._Plan()
            self._layout(pl, E, B, shapes, hw2, nhwc)
            return pl
        return layout

    def _measure(self, dims):
        return measure_bytes(self._layout_for(dims))

    def reserve(self, batch, shapes, hw2, slots=(0,), orig_sizes=()):
        """Size the arenas of `slots` up front for a feature pyramid (`shapes`: the three
        coarse levels low -> high resolution, `hw2`: the 1/4-resolution level) of `batch`
        images and, with `orig_sizes` [(H0, W0)], for post-processing at those original image
        sizes.  Optional: an arena also grows on demand (one device wait each time its
        envelope grows); a loop that knows its largest shapes -- Resize(img_scale=(1333, 800)):
        800 x 1333 and 1333 x 800 -- reserves them once and never waits."""
        if self.w is None:
            self._pack()
        dims = self._plan_dims(batch, shapes, hw2)
        for s in slots:
            self._arena(s).reserve(dims, self._measure)
            if orig_sizes:
                self._post_arena(s).reserve(
                    (batch, max(h * w for h, w in orig_sizes)),
                    lambda d: measure_bytes(lambda E: self._post_layout(E, [(1, d[1])] * d[0])))

    def arena_bytes(self):
        """Device bytes held by the slots' arenas (what the plans are views of)."""
        return sum(a.capacity for t in (self._arenas, self._post_arenas) for a in t.values())

    def _plan(self, B, shapes, hw2, slot=0, nhwc=False):
        key = (B, tuple(shapes), tuple(hw2), slot, getattr(self, "return_all_layers", False),
               nhwc)
        if key in self._plans:
            return self._plans[key]
        if self.w is None:
            self._pack()

        dims = self._plan_dims(B, shapes, hw2)
        pl = self._arena(slot).carve(self._layout_for(dims, nhwc), dims, self._measure)
        pl.slot, pl.key = slot, key
        pl.graph_a = pl.graph_b = pl.static_feats = pl.graph_cfg = pl.feats_read = None
        pl.graph_c = PlanCache(self.POST_VIEWS)
        pl.post_views = OrderedDict()
        pl.static_ptrs = None
        pl.graphs_a = OrderedDict()
        pl.calls_a = pl.calls_b = 0
        pl.streams = {}
        pl.enc_pos, pl.dec_kpos, pl.pe_ready, pl.enc_pos8 = self._position_tables(shapes)
        pl.pe_waited = False
        c = self._const(B)
        if c["me0"] is None:
            # the mask embedding of the INITIAL queries: a function of the weights alone,
            # computed once per batch size on PRIVATE scratch outside the arena -- this plan's
            # arena views alias the buffers of the slot's previous batch, which may still be
            # executing on another stream when a plan of a new batch size is first built
            # (complete before any other stream can read it: one host wait per state dict)
            from types import SimpleNamespace
            BQ = B * self.num_obj_query
            tmp = SimpleNamespace(B=B, cls=None, MP=None,
                                  **{n: torch.empty(BQ, 256, device=self.device)
                                     for n in ("qn", "m1", "m2", "me")})
            self._head_embed(pl.q0, tmp, False, False)
            c["me0"] = tmp.me
            torch.cuda.current_stream(self.device).synchronize()
        pl.me0 = c["me0"]
        self._plans[key] = pl
        return pl

    def _layout(self, pl, E, B, shapes, hw2, nhwc):
        """Every per-image buffer of the head as views of one arena (`E(*shape)` carves a
        float32 view).  Sizes are non-decreasing in B and in every height / width, so a plan
        of any shape within the arena's envelope fits (plans.py)."""
        pl.B, pl.shapes, pl.hw2, pl.nhwc = B, list(shapes), tuple(hw2), nhwc
        pl.N = [h * w for h, w in shapes]
        pl.start = [0, pl.N[0], pl.N[0] + pl.N[1]]
        pl.SN = sum(pl.N)
        SN, Q, R = pl.SN, self.num_obj_query, self.num_rel_query
        HW2 = hw2[0] * hw2[1]
        pl.HW2 = HW2
        M = B * SN
        # ---- pixel decoder ----
        pl.X, pl.X1, pl.Y = E(B, SN, 256), E(B, SN, 256), E(B, SN, 256)
        pl.S = E(B, SN, 256)
        pl.VOA = E(B, SN, 544)          # [value | offsets | logits] per token
        pl.H = E(M, self.enc_ffn)
        # S3 operands of the encoder (gemm_arithmetic == "bf16x3"): tokens, tokens + positions,
        # sampled values, the norms.0 output; the FFN's hidden rows live in pl.H (6 of its 4 bytes
        # per element would not fit: its own buffer)
        pl.XS, pl.XPS = E(hip.s3_floats(M, 256)), E(hip.s3_floats(M, 256))
        pl.SS, pl.X1S = E(hip.s3_floats(M, 256)), E(hip.s3_floats(M, 256))
        pl.HS = E(hip.s3_floats(M, self.enc_ffn))
        pl.tmpconv = E(B, max(pl.N), 256)
        pl.splitk = E(B * 9 * 1024 * 1024)   # split-K workspace of the C5 / C4 input convs
        nblk = max(hip.groupnorm_nblk(HW2), hip.groupnorm_nblk(max(pl.N)))
        pl.gn_part = E.f64(B * nblk * 32 * 2)
        pl.T1, pl.T2 = E(B, HW2, 256), E(B, HW2, 256)
        # (grouped input convolutions: one output buffer per level, views of pl.T1, which is
        # idle until the lateral convolution: sum(N) <= HW2 rows)
        pl.tmpconv3 = None
        if sum(pl.N) <= HW2:
            t1 = pl.T1.view(-1)
            offs = [0, B * pl.N[0] * 256, B * (pl.N[0] + pl.N[1]) * 256]
            pl.tmpconv3 = [t1[o:o + B * n * 256].view(B, n, 256) for o, n in zip(offs, pl.N)]
        # Winograd scratch: F(2x2): 16 planes of B * HW2 / 4 tiles x 256 (even sides only),
        # F(4x4): 36 planes of B * ceil(H2/4) * ceil(W2/4) tiles x 256 (sized for both, whatever
        # the parity of this shape: the arena's envelope must cover every shape below it)
        pl.wino = hw2[0] % 2 == 0 and hw2[1] % 2 == 0
        t4 = B * ((hw2[0] + 3) // 4) * ((hw2[1] + 3) // 4)
        t2 = B * ((hw2[0] + 1) // 2) * ((hw2[1] + 1) // 2)
        n = max(16 * t2, 36 * t4) * 256
        pl.wV, pl.wM = E(n), E(n)
        pl.MF = E(B, HW2, 256)
        # ---- decoder ----
        nd = self.num_dec_layers
        pl.Kp = [E(B, pl.N[i % 3], 256) for i in range(nd)]
        pl.Vp = [E(B, pl.N[i % 3], 256) for i in range(nd)]
        BQ = B * Q
        pl.q, pl.q1, pl.q2, pl.qy = E(BQ, 256), E(BQ, 256), E(BQ, 256), E(BQ, 256)
        pl.q0 = self._const(B)["q0"]
        pl.qn, pl.m1, pl.m2, pl.me = E(BQ, 256), E(BQ, 256), E(BQ, 256), E(BQ, 256)
        pl.Qp, pl.att, pl.Qp0 = E(BQ, 256), E(BQ, 256), E(BQ, 256)
        pl.VQK = E(BQ, 768)
        pl.MFd = [E(B, n, 256) for n in pl.N]    # mask feature resampled to each level
        pl.MFs = [E(B, 4 * n, 256) for n in pl.N]   # exact_mask_order=True: stencil rows ...
        pl.ML4 = E(BQ, 4 * max(pl.N))               # ... and their logits
        pl.hq = E(hip.ffn_scratch_floats(BQ, self.dec_ffn))
        pl.MP = E(B, Q, HW2)
        pl.ML = E(BQ, max(pl.N))
        pl.bits = E.i32(BQ * ((max(pl.N) + 31) // 32))
        pl.rowall = E.i32(BQ)
        pl.cls = E(B, Q, self.num_classes + 1)
        self._plan_relation(pl, E)

    def _plan_relation(self, pl, E):
        """Buffers of the Pair Proposal Network and the Relation Fusion decoder."""
        B, Q, R = pl.B, self.num_obj_query, self.num_rel_query
        BQ, HW2 = B * Q, pl.HW2
        scr = max(hip.attn_scratch_floats(B, Q, n) for n in pl.N + [Q])
        scr = max(scr, hip.attn_scratch_floats(B, R, 2 * R), hip.attn_scratch_floats(B, R, R))
        pl.scr = E(scr)
        # ---- PPN ----
        pl.s1, pl.s2, pl.sn, pl.on = E(BQ, 256), E(BQ, 256), E(BQ, 256), E(BQ, 256)
        pl.imp_raw, pl.imp = E(B, Q, Q), E(B, Q, Q)
        pl.c1, pl.c2 = E(B, Q * Q, 64), E(B, Q * Q, 64)
        # split-K workspace of the 64 -> 64 Matrix Learner layer (few output tiles, K = 3136)
        tiles = B * ((Q * Q + 63) // 64)
        pl.ppn_splitk = E(8 * B * Q * Q * 64) if tiles < 512 else None
        pl.topk_idx, pl.sub_pos, pl.obj_pos = E.i64(B, R), E.i64(B, R), E.i64(B, R)
        pl.pair_idx = E.i64(B, 2 * R)
        pl.pair = E(B * 2 * R, 256)
        # ---- relation decoder ----
        BR = B * R
        pl.r, pl.r1, pl.r2, pl.ry = E(BR, 256), E(BR, 256), E(BR, 256), E(BR, 256)
        pl.r0 = self._const(B).get("r0")
        pl.rQp, pl.ratt = E(BR, 256), E(BR, 256)
        pl.rVQK = E(BR, 768)
        pl.rh = E(hip.ffn_scratch_floats(BR, self.rel_ffn))
        pl.pVK = E(B * 2 * R, 512)
        pl.pVK_all = [E(B * 2 * R, 512) for _ in range(self.num_rel_layers)]
        pl.rQp0 = None
        pl.rel = E(B, R, self.num_relations)
        pl.sub_cls, pl.obj_cls = E(B, R, self.num_classes + 1), E(B, R, self.num_classes + 1)
        pl.sub_seg, pl.obj_seg = E(B, R, HW2), E(B, R, HW2)

    # ----------------------------------------------------------- sub-graphs
    def _pixel_decoder(self, feats, pl):
        """MSDeformAttnPixelDecoder -> pl.X (memories), pl.MF."""
        w, B, SN = self.w, pl.B, pl.SN
        pd = "pixel_decoder."
        group = self.group_input_convs and pl.nhwc and pl.tmpconv3 is not None
        if group:
            # the three 1x1 input convolutions (C5 / C4 / C3: 68 + 264 + 1044 tiles with 64 / 32 /
            # 16 k-chunks) as ONE grouped launch instead of three split-K launches and their
            # three reduce passes (channels_last features are row-major A operands)
            hip.gemm_group([dict(
                A=feats[3 - l], W=w[pd + "input_convs.%d.conv.weight" % l], C=pl.tmpconv3[l],
                M=pl.N[l], N=256, K=feats[3 - l].shape[1], lda=feats[3 - l].shape[1],
                ldw=feats[3 - l].shape[1], ldc=256, bias=w[pd + "input_convs.%d.conv.bias" % l],
                batch=B, sA=feats[3 - l].shape[1] * pl.N[l], sC=pl.N[l] * 256) for l in range(3)])
        for l in range(3):
            f = feats[3 - l]
            cin, n = f.shape[1], pl.N[l]
            # NCHW features are read as column-major A operands, channels_last ones as
            # row-major [pixels][channels]: no transpose pass either way
            conv = pl.tmpconv3[l] if group else pl.tmpconv
            if not group:
                hip.gemm(f, w[pd + "input_convs.%d.conv.weight" % l], conv, M=n, N=256, K=cin,
                         lda=cin if pl.nhwc else n, ldw=cin, ldc=256,
                         bias=w[pd + "input_convs.%d.conv.bias" % l], batch=B, sA=cin * n,
                         sC=n * 256, colmajor=not pl.nhwc, scratch=pl.splitk)
            hip.groupnorm_nhwc(conv, w[pd + "input_convs.%d.gn.weight" % l],
                               w[pd + "input_convs.%d.gn.bias" % l], pl.X[:, pl.start[l]:],
                               pl.gn_part, B, n, self.gn_groups, False, n * 256, SN * 256)
        X2, X12, Y2 = pl.X.view(-1, 256), pl.X1.view(-1, 256), pl.Y.view(-1, 256)
        if self.gemm_arithmetic == "bf16x3":
            self._encoder_s3(pl)
        else:
            self._encoder_fp32(pl)
        # FPN level (C2): lateral 1x1 + GN, + bilinear-up(finest memory), 3x3 + GN + ReLU
        f = feats[0]
        cin, HW2 = f.shape[1], pl.HW2
        H2, W2 = pl.hw2
        hip.gemm(f, w[pd + "lateral_convs.0.conv.weight"], pl.T1, M=HW2, N=256, K=cin,
                 lda=cin if pl.nhwc else HW2, ldw=cin, ldc=256, batch=B, sA=cin * HW2,
                 sC=HW2 * 256, colmajor=not pl.nhwc)
        h2, w2 = pl.shapes[2]
        if getattr(self, "fuse_lateral_upadd", False):
            hip.groupnorm_upadd_nhwc(pl.T1, w[pd + "lateral_convs.0.gn.weight"],
                                     w[pd + "lateral_convs.0.gn.bias"], pl.T2, pl.gn_part,
                                     pl.X[:, pl.start[2]:], B, H2, W2, h2, w2, self.gn_groups,
                                     HW2 * 256, HW2 * 256, SN * 256)
        else:
            hip.groupnorm_nhwc(pl.T1, w[pd + "lateral_convs.0.gn.weight"],
                               w[pd + "lateral_convs.0.gn.bias"], pl.T2, pl.gn_part, B, HW2,
                               self.gn_groups, False, HW2 * 256, HW2 * 256)
            hip.bilinear_nhwc(pl.X[:, pl.start[2]:], pl.T2, B, h2, w2, H2, W2, 256, True, SN * 256,
                              HW2 * 256)
        if self.conv_algo == "winograd4":
            hip.conv3x3_winograd43(pl.T2, w[pd + "output_convs.0.conv.winograd4"], None, pl.T1,
                                   pl.wV, pl.wM, B, H2, W2, 256, 256, False)
        elif pl.wino and self.conv_algo == "winograd":
            hip.conv3x3_winograd(pl.T2, w[pd + "output_convs.0.conv.winograd"], None, pl.T1,
                                 pl.wV, pl.wM, B, H2, W2, 256, 256, False)
        else:
            hip.conv2d_nhwc(pl.T2, w[pd + "output_convs.0.conv.weight"], None, pl.T1, B, H2, W2,
                            256, 256, 3, 3, 1, False)
        hip.groupnorm_nhwc(pl.T1, w[pd + "output_convs.0.gn.weight"],
                           w[pd + "output_convs.0.gn.bias"], pl.T2, pl.gn_part, B, HW2,
                           self.gn_groups, True, HW2 * 256, HW2 * 256)
        hip.linear(pl.T2.view(-1, 256), w[pd + "mask_feature.weight"], w[pd + "mask_feature.bias"],
                   pl.MF.view(-1, 256))
        if not self.exact_mask_order:
            for l, (h, wd) in enumerate(pl.shapes):
                hip.bilinear_nhwc(pl.MF, pl.MFd[l], B, H2, W2, h, wd, 256, False, HW2 * 256,
                                  pl.N[l] * 256)
        elif self.exact_mask_order != "full" and not self._gathers_stencil():
            # the mask-feature rows each level's bilinear stencils read, once per image
            for l, (h, wd) in enumerate(pl.shapes):
                hip.bilinear_stencil_rows(pl.MF, pl.MFs[l], B, H2, W2, h, wd, 256, HW2 * 256,
                                          4 * pl.N[l] * 256)

    def _gathers_stencil(self):
        return bool(self.exact_mask_order and self.exact_mask_order != "full" and
                    self.fuse_mask_pack and getattr(self, "gather_mask_stencil", True))

    def _encoder_fp32(self, pl):
        """The six encoder layers on the exact-fp32 MFMA kernels (rounds 1-5)."""
        w, B, SN = self.w, pl.B, pl.SN
        pd = "pixel_decoder."
        X2, X12, Y2 = pl.X.view(-1, 256), pl.X1.view(-1, 256), pl.Y.view(-1, 256)
        for i in range(self.num_enc_layers):
            p = pd + "encoder.layers.%d." % i
            a = p + "attentions.0."
            hip.gemm(X2, w[a + "voa.weight"], pl.VOA, M=B * SN, N=544, K=256, lda=256, ldw=256,
                     ldc=544, bias=w[a + "voa.bias"], aadd=pl.enc_pos, ldaadd=256, aadd_rows=SN,
                     aadd_from_col=256)
            hip.msda(pl.VOA, 544, pl.VOA.view(-1)[256:], 544, pl.S, B, pl.shapes)
            # output_proj + identity + norms.0, and ffns.0.layers.1 + identity + norms.1: each
            # one launch whose workgroups own whole rows (csrc/gemm_ln.hip; bitwise the
            # GEMM -> LayerNorm pair it replaces, `enc_fused_ln` selects per site)
            if "proj" in self.enc_fused_ln:
                hip.linear_res_ln(pl.S.view(-1, 256), w[a + "output_proj.weight"],
                                  w[a + "output_proj.bias"], X2, w[p + "norms.0.weight"],
                                  w[p + "norms.0.bias"], X12)
            else:
                hip.linear(pl.S.view(-1, 256), w[a + "output_proj.weight"],
                           w[a + "output_proj.bias"], Y2, res=X2)
                hip.layernorm(Y2, w[p + "norms.0.weight"], w[p + "norms.0.bias"], X12)
            hip.linear(X12, w[p + "ffns.0.layers.0.0.weight"], w[p + "ffns.0.layers.0.0.bias"],
                       pl.H, relu=True)
            if "ffn" in self.enc_fused_ln:
                hip.linear_res_ln(pl.H, w[p + "ffns.0.layers.1.weight"],
                                  w[p + "ffns.0.layers.1.bias"], X12, w[p + "norms.1.weight"],
                                  w[p + "norms.1.bias"], X2)
            else:
                hip.linear(pl.H, w[p + "ffns.0.layers.1.weight"], w[p + "ffns.0.layers.1.bias"],
                           Y2, res=X12)
                hip.layernorm(Y2, w[p + "norms.1.weight"], w[p + "norms.1.bias"], X2)

    def _encoder_s3(self, pl):
        """The six encoder layers with their GEMMs on the bf16 matrix pipe (csrc/gemm_s3.hip).
        Activations travel between the GEMMs as S3 operands (three exact bf16 planes) written by
        the producing kernel's epilogue: XS = tokens, XPS = tokens + positions (the reference's
        `query + query_pos`), X1S = norms.0 output, HS = FFN hidden rows; residuals are read back
        from those planes (exact).  fp32 rows exist where a non-GEMM consumer reads them: VOA (the
        sampling kernel) and the final memory pl.X -- and S, the sampling kernel's output, which
        output_proj reads as rows (`enc_proj_reads_rows`).  Live per layer with the default
        switches: XS, XPS, VOA, S, X1S; SS (the split of S) is written only with
        `enc_proj_reads_rows` off or `msda_s3_out` on, HS only with `fuse_encoder_ffn` off: both
        stay carved either way."""
        w, B, SN = self.w, pl.B, pl.SN
        pd = "pixel_decoder."
        M, F = B * SN, self.enc_ffn
        X2 = pl.X.view(-1, 256)
        pos8 = (pl.enc_pos8, SN)
        # the one-launch FFN handles a hidden width that is a multiple of 256 (the config's 1024)
        fuse_ffn = bool(getattr(self, "fuse_encoder_ffn", 0)) and F % 256 == 0
        rows_proj = bool(getattr(self, "enc_proj_reads_rows", 0)) and not self.msda_s3_out
        hip.s3_split(X2, pl.XS, add=pl.enc_pos, out_add=pl.XPS)      # one read of the tokens
        for i in range(self.num_enc_layers):
            p = pd + "encoder.layers.%d." % i
            a = p + "attentions.0."
            last = i + 1 == self.num_enc_layers
            hip.gemm_s3(pl.XS, w[a + "voa.weight.s3"], M, 544, 256, bias=w[a + "voa.bias"],
                        out=pl.VOA.view(-1, 544), a2=pl.XPS, a2_from_col=256)
            if self.msda_s3_out:
                hip.msda(pl.VOA, 544, pl.VOA.view(-1)[256:], 544, pl.SS, B, pl.shapes, s3_out=True)
            else:
                hip.msda(pl.VOA, 544, pl.VOA.view(-1)[256:], 544, pl.S, B, pl.shapes)
                if not rows_proj:
                    hip.s3_split(pl.S.view(-1, 256), pl.SS)
            proj = dict(bias=w[a + "output_proj.bias"], out_s3=pl.X1S, res_s3=pl.XS,
                        gamma=w[p + "norms.0.weight"], beta=w[p + "norms.0.bias"])
            if rows_proj:                # (pl.SS stays carved and is not written)
                hip.gemm_s3_rows_ln(pl.S.view(-1, 256), w[a + "output_proj.weight.s3"], M, 256, 256,
                                    **proj)
            else:
                hip.gemm_s3(pl.SS, w[a + "output_proj.weight.s3"], M, 256, 256, **proj)
            tail = dict(res_s3=pl.X1S, gamma=w[p + "norms.1.weight"], beta=w[p + "norms.1.bias"],
                        out=X2 if last else None, out_s3=None if last else pl.XS,
                        out_s3_pos=None if last else pl.XPS, pos=pos8)
            if fuse_ffn:                 # (pl.HS stays carved and is not written)
                hip.gemm_s3_ffn(pl.X1S, w[p + "ffns.0.layers.0.0.weight.s3"],
                                w[p + "ffns.0.layers.1.weight.s3"], M, 256, 256, F,
                                b1=w[p + "ffns.0.layers.0.0.bias"],
                                b2=w[p + "ffns.0.layers.1.bias"], **tail)
                continue
            hip.gemm_s3(pl.X1S, w[p + "ffns.0.layers.0.0.weight.s3"], M, F, 256,
                        bias=w[p + "ffns.0.layers.0.0.bias"], relu=True, out_s3=pl.HS)
            hip.gemm_s3(pl.HS, w[p + "ffns.0.layers.1.weight.s3"], M, 256, F,
                        bias=w[p + "ffns.0.layers.1.bias"], **tail)

    def _mlp3(self, prefix, src, dst, pl):
        """Linear-ReLU-Linear-ReLU-Linear (`mask_embed`-style heads) via pl.m1 / pl.m2."""
        w = self.w
        hip.linear(src, w[prefix + ".0.weight"], w[prefix + ".0.bias"], pl.m1, relu=True)
        hip.linear(pl.m1, w[prefix + ".2.weight"], w[prefix + ".2.bias"], pl.m2, relu=True)
        hip.linear(pl.m2, w[prefix + ".4.weight"], w[prefix + ".4.bias"], dst)

    def _mask_logits(self, me, pl, out):
        """out[b, q, :] = me[b, q, :] . MF[b, :, :]^T  (`einsum("bqc,bchw->bqhw")`)."""
        Q = self.num_obj_query
        hip.gemm(me, pl.MF, out, M=Q, N=pl.HW2, K=256, lda=256, ldw=256, ldc=pl.HW2,
                 batch=pl.B, sA=Q * 256, sW=pl.HW2 * 256, sC=Q * pl.HW2)

    def _head_embed(self, q, pl, with_cls, full_mask, cls_out=None, mp_out=None, normed=False):
        """post_norm -> (cls_embed) -> mask_embed MLP -> pl.me; with `full_mask` also the
        mask logits [B,Q,H2*W2] (pairnet_head.py:236-243).  Outputs go to pl.cls / pl.MP
        unless other destinations are given."""
        w, B, Q = self.w, pl.B, self.num_obj_query
        cls_out = pl.cls if cls_out is None else cls_out
        mp_out = pl.MP if mp_out is None else mp_out
        if not normed:   # (`normed`: pl.qn already holds post_norm(q), from the FFN kernel)
            hip.layernorm(q, w["transformer_decoder.post_norm.weight"],
                          w["transformer_decoder.post_norm.bias"], pl.qn)
        if with_cls:
            hip.linear(pl.qn, w["cls_embed.weight"], w["cls_embed.bias"], cls_out.view(B * Q, -1))
        self._mlp3("mask_embed", pl.qn, pl.me, pl)
        if full_mask:
            self._mask_logits(pl.me, pl, mp_out)

    def _attn_mask(self, pl, lvl, mp=None, me=None):
        """Boolean attention mask of level `lvl` + all-masked fix (pairnet_head.py:244-256,
        :300) -> pl.bits / pl.rowall.

        The reference resizes the full-resolution mask logits bilinearly and thresholds.
        `exact_mask_order`:
          False   bilinear resampling is linear, so resize(me . MF) == me . resize(MF): the
                  mask feature is resampled once per image (pl.MFd) and each layer's logits
                  are a Q x N_l GEMM (same values up to fp32 re-association);
          True    the reference's operation order, computed sparsely: an output pixel's
                  bilinear stencil reads 4 full-resolution logits, so the layer computes
                  exactly those -- me against the 4 N_l stencil rows of the mask feature
                  (pl.MFs, gathered once per image; the same tile GEMM, hence the same
                  rounding per logit, as the full Q x H2 W2 product) -- and
                  `pn_mask_pack_stencil` blends them like `pn_bilinear_planar_f32`;
          "full"  the dense form of the same thing (full-resolution logits, planar resize,
                  pack): bit for bit the result of True, kept as its cross-check."""
        B, Q = pl.B, self.num_obj_query
        h, wd = pl.shapes[lvl]
        n = h * wd
        if self.exact_mask_order == "full":
            hip.bilinear_planar(pl.MP if mp is None else mp, pl.ML, B * Q, pl.hw2[0], pl.hw2[1],
                                h, wd)
        elif self.exact_mask_order and self.fuse_mask_pack:
            # logits, blend, threshold and pack in ONE launch: the same products in the same
            # order as the pair below (bit-identical bits), without the Q x 4 N_l logit map
            if self._gathers_stencil():
                hip.mask_stencil_gather_gemm(pl.me if me is None else me, pl.MF, pl.bits,
                                             pl.rowall, B, Q, pl.hw2[0], pl.hw2[1], h, wd)
            else:
                hip.mask_stencil_gemm(pl.me if me is None else me, pl.MFs[lvl], pl.bits,
                                      pl.rowall, B, Q, pl.hw2[0], pl.hw2[1], h, wd)
            return
        elif self.exact_mask_order:
            hip.gemm(pl.me if me is None else me, pl.MFs[lvl], pl.ML4, M=Q, N=4 * n, K=256,
                     lda=256, ldw=256, ldc=4 * n, batch=B, sA=Q * 256, sW=4 * n * 256,
                     sC=Q * 4 * n, force="tile64")
            hip.mask_pack_stencil(pl.ML4, pl.bits, pl.rowall, B * Q, pl.hw2[0], pl.hw2[1], h, wd)
            return
        else:
            hip.gemm(pl.me if me is None else me, pl.MFd[lvl], pl.ML, M=Q, N=n, K=256, lda=256,
                     ldw=256, ldc=n, batch=B, sA=Q * 256, sW=n * 256, sC=Q * n)
        hip.mask_pack(pl.ML, pl.bits, pl.rowall, B * Q, n)

    def _layer(self, pre, x, xpos, x1, x2, y, Qp, VQK, att, hbuf, Kp, ldk, Vp, ldv, Nk, B, nq,
               bits, rowall, scr, ffn, self_first=False, post=None, x_in=None):
        """One post-norm decoder layer (facebook_detr.py:378-432 semantics); x is updated
        in place.  Operation order (cross_attn, norm, self_attn, norm, ffn, norm), or with
        `self_first` (self_attn, norm, cross_attn, norm, ffn, norm); attentions.<j> is the
        j-th attention in that order, as mmcv's BaseTransformerLayer numbers them.  `x_in`:
        read the layer's input from there instead of x (the first layer reads the constant
        initial queries in place: no per-image copy into x)."""
        w = self.w
        scale = 1.0 / math.sqrt(32.0)
        ac = pre + "attentions.%d.attn." % (1 if self_first else 0)
        as_ = pre + "attentions.%d.attn." % (0 if self_first else 1)
        nc, ns = ("norms.1.", "norms.0.") if self_first else ("norms.0.", "norms.1.")

        def cross(src, dst):
            hip.linear(src, w[ac + "in_proj_weight"][:256], w[ac + "in_proj_bias"][:256], Qp,
                       aadd=xpos)
            hip.attention(Qp, 256, Kp, ldk, Vp, ldv, bits, rowall, att, 256, scr, B, nq, Nk, scale)
            hip.linear(att, w[ac + "out_proj.weight"], w[ac + "out_proj.bias"], y, res=src)
            hip.layernorm(y, w[pre + nc + "weight"], w[pre + nc + "bias"], dst)

        def self_attn(src, dst):
            hip.linear(src, w[as_ + "vqk.weight"], w[as_ + "vqk.bias"], VQK, aadd=xpos,
                       aadd_from_col=256)
            hip.attention(VQK[:, 256:], 768, VQK[:, 512:], 768, VQK, 768, None, None, att, 256,
                          scr, B, nq, nq, scale)
            hip.linear(att, w[as_ + "out_proj.weight"], w[as_ + "out_proj.bias"], y, res=src)
            hip.layernorm(y, w[pre + ns + "weight"], w[pre + ns + "bias"], dst)

        x_in = x if x_in is None else x_in
        if self_first:
            self_attn(x_in, x1)
            cross(x1, x2)
        else:
            cross(x_in, x1)
            self_attn(x1, x2)
        hip.ffn_ln(x2, w[pre + "ffns.0.layers.0.0.weight"], w[pre + "ffns.0.layers.0.0.bias"],
                   w[pre + "ffns.0.layers.1.weight"], w[pre + "ffns.0.layers.1.bias"],
                   w[pre + "norms.2.weight"], w[pre + "norms.2.bias"], x, hbuf, B * nq, ffn,
                   post=post)

    # --------------------------------------------------------------- forward
    # Stage A: everything that does not depend on the query chain (pixel decoder, the
    # mask-feature resampling, the K/V projections of all nine decoder layers): a few
    # dozen large, chip-filling launches.
    def _stage_a(self, feats, pl):
        with hip.reserve_slots(self.grid_reserve):
            self._stage_a_launches(feats, pl)

    def _stage_a_launches(self, feats, pl):
        self._pixel_decoder(feats, pl)
        # K / V projections of all decoder layers up front (query-independent), as grouped
        # launches: 18 problems whose tile counts (9/33/131 x 2 per image) would each
        # leave most of the 256 CUs idle on their own
        probs = self._kv_problems(pl)
        for j in range(0, len(probs), hip.GEMM_GROUP_MAX):
            hip.gemm_group(probs[j:j + hip.GEMM_GROUP_MAX])

    def _memory_kv(self, pl, attn_prefix, l, Kp, Vp):
        """The two GEMM problems K = (mem_l + level_embed_l + pe_l) Wk^T + bk and
        V = (mem_l + level_embed_l) Wv^T + bv of one cross-attention over level l."""
        w, B = self.w, pl.B
        mem = pl.X[:, pl.start[l]:]
        common = dict(A=mem, M=pl.N[l], N=256, K=256, lda=256, ldw=256, ldc=256, batch=B,
                      sA=pl.SN * 256, sC=pl.N[l] * 256, ldaadd=256)
        return [dict(W=w[attn_prefix + "in_proj_weight"][256:512], C=Kp,
                     bias=w[attn_prefix + "in_proj_bias"][256:512], aadd=pl.dec_kpos[l],
                     aadd_rows=pl.N[l], **common),
                dict(W=w[attn_prefix + "in_proj_weight"][512:], C=Vp,
                     bias=w[attn_prefix + "in_proj_bias"][512:],
                     aadd=w["level_embed.weight"][l:l + 1], aadd_rows=1, **common)]

    def _kv_problems(self, pl):
        probs = []
        for i in range(self.num_dec_layers):
            probs += self._memory_kv(pl, "transformer_decoder.layers.%d.attentions.0.attn." % i,
                                     i % 3, pl.Kp[i], pl.Vp[i])
        return probs

    # Stage B: the sequential query chain (9 masked decoder layers, PPN, top-k, 6 relation
    # layers, output gathers): ~200 small latency-bound launches.
    def _stage_b(self, pl):
        self._object_decoder(pl)
        self._relation_stage(pl)

    def _object_decoder(self, pl, all_layers=False, final_head=True):
        """The 9 masked-attention layers (pairnet_head.py:289-320) -> pl.q, pl.cls, pl.MP;
        with `all_layers` every layer's class / mask logits go to pl.cls_all / pl.MP_all;
        without `final_head` the last layer's class / mask heads are left to the caller."""
        w, B, Q = self.w, pl.B, self.num_obj_query
        qpos = w["query_embed.weight"]
        exact = self.exact_mask_order == "full"     # full-resolution logits of every layer
        # the INITIAL queries are learned constants (pl.q0: `query_feat` repeated over the
        # batch; the first layer reads them in place), and so is their mask embedding pl.me0:
        # both live in `_const(B)`, outside the arenas (a new state dict drops them)
        if exact:
            self._head_embed(pl.q0, pl, False, True)
        last = self.num_dec_layers - 1
        mp = None
        # post_norm of every layer's output comes out of the layer's FFN kernel
        post = (w["transformer_decoder.post_norm.weight"], w["transformer_decoder.post_norm.bias"],
                pl.qn)
        for i in range(self.num_dec_layers):
            l = i % 3
            self._attn_mask(pl, l, mp, me=pl.me0 if (i == 0 and not exact) else None)
            self._layer("transformer_decoder.layers.%d." % i, pl.q, qpos, pl.q1, pl.q2, pl.qy,
                        pl.Qp, pl.VQK, pl.att, pl.hq, pl.Kp[i], 256, pl.Vp[i], 256, pl.N[l], B,
                        Q, pl.bits, pl.rowall, pl.scr, self.dec_ffn, post=post,
                        x_in=pl.q0 if i == 0 else None)
            if all_layers:
                mp = pl.MP_all[i]
                self._head_embed(pl.q, pl, True, True, pl.cls_all[i], mp, normed=True)
            elif final_head:
                self._head_embed(pl.q, pl, i == last, exact or i == last, normed=True)
            elif i != last:
                self._head_embed(pl.q, pl, False, exact, normed=True)

    def _relation_stage(self, pl):
        self._pair_proposal(pl)
        self._relation_decoder(pl)

    def _pair_proposal(self, pl):
        """Pair Proposal Network (pairnet_head.py:322-351): pl.q -> pl.imp_raw, pl.imp,
        pl.topk_idx / sub_pos / obj_pos and the gathered pair features pl.pair."""
        w, B, Q, R = self.w, pl.B, self.num_obj_query, self.num_rel_query
        for mlp, dst in (("sub_query_update", pl.sn), ("obj_query_update", pl.on)):
            hip.linear(pl.q, w[mlp + ".0.weight"], w[mlp + ".0.bias"], pl.s1, relu=True)
            hip.linear(pl.s1, w[mlp + ".2.weight"], w[mlp + ".2.bias"], pl.s2, relu=True)
            if self.fuse_ppn_front:    # un-normalised: k_ppn_front normalises while staging
                hip.linear(pl.s2, w[mlp + ".4.weight"], w[mlp + ".4.bias"], dst)
                continue
            hip.linear(pl.s2, w[mlp + ".4.weight"], w[mlp + ".4.bias"], pl.s1)
            hip.l2normalize(pl.s1, dst)
        ml = "update_importance.conv_layers."
        if self.fuse_ppn_front:
            hip.ppn_front(pl.sn, pl.on, w[ml + "0.0.weight"], w[ml + "0.0.bias"], pl.imp_raw,
                          pl.c1, B, Q)
        else:
            hip.gemm(pl.sn, pl.on, pl.imp_raw, M=Q, N=Q, K=256, lda=256, ldw=256, ldc=Q, batch=B,
                     sA=Q * 256, sW=Q * 256, sC=Q * Q)
            hip.mlearner_first(pl.imp_raw, w[ml + "0.0.weight"], w[ml + "0.0.bias"], pl.c1, B, Q)
        # (157 output tiles x K = 3136 at Q = 100: the K contraction is split, which takes the
        # layer from 112 to ~45 us on the dependent chain)
        hip.conv2d_ex(pl.c1, w[ml + "1.0.weight"], w[ml + "1.0.bias"], None, pl.c2, B, Q, Q, 64,
                      64, 7, 7, 1, 3, relu=True, scratch=pl.ppn_splitk)
        hip.mlearner_last(pl.c2, w[ml + "2.0.weight"], w[ml + "2.0.bias"], pl.imp, B, Q)
        hip.topk_pairs(pl.imp, pl.topk_idx, pl.sub_pos, pl.obj_pos, B, Q, R, pair=pl.pair_idx)
        # ---- pair features (:342-351) ----
        hip.gather_rows(pl.q, pl.pair_idx, pl.pair, B, Q, 2 * R, 256)

    def _relation_decoder(self, pl):
        """Relation Fusion decoder (pairnet_head.py:353-378) over pl.pair ([B][sub R | obj R]
        rows) -> pl.rel, then the output gathers (:380-403)."""
        w, B, Q, R = self.w, pl.B, self.num_obj_query, self.num_rel_query
        rpos, ppos = w["rel_query_embed.weight"], w["rel_query_embed2.weight"]
        # the pair features' [V | K] projections of all six layers (layer-independent input):
        # one grouped launch
        hip.gemm_group([dict(
            A=pl.pair, W=w["relation_decoder.layers.%d.attentions.0.attn.vk.weight" % i],
            C=pl.pVK_all[i], bias=w["relation_decoder.layers.%d.attentions.0.attn.vk.bias" % i],
            M=B * 2 * R, N=512, K=256, lda=256, ldw=256, ldc=512, aadd=ppos, ldaadd=256,
            aadd_rows=2 * R, aadd_from_col=256) for i in range(self.num_rel_layers)])
        for i in range(self.num_rel_layers):
            pre = "relation_decoder.layers.%d." % i
            pvk = pl.pVK_all[i]
            self._layer(pre, pl.r, rpos, pl.r1, pl.r2, pl.ry, pl.rQp, pl.rVQK, pl.ratt, pl.rh,
                        pvk[:, 256:], 512, pvk, 512, 2 * R, B, R, None, None, pl.scr,
                        self.rel_ffn, x_in=pl.r0 if i == 0 else None)
        hip.linear(pl.r, w["rel_cls_embed.weight"], w["rel_cls_embed.bias"], pl.rel.view(B * R, -1))
        self._gather_outputs(pl)

    # (the sibling heads select their pairs and build their masks differently: they keep the
    # gathered logits)
    _pair_masks_fusable = True

    def _fused_pair_masks(self):
        # (pn_pair_masks_u8 takes 2R <= 2048, Q <= 65535: the constructor's num_rel_query <= 128,
        # num_obj_query <= 256 are far inside)
        return self._pair_masks_fusable and bool(getattr(self, "fused_pair_masks", True))

    def _gather_outputs(self, pl):
        """The subject / object gathers of the selected pairs (pairnet_head.py:380-403).  With
        `fused_pair_masks` the mask logits stay where they are: `_get_bboxes_single` reads
        MP[sub_pos] / MP[obj_pos] in place, `forward()` gathers them for its caller."""
        B, Q, R = pl.B, self.num_obj_query, self.num_rel_query
        nc = self.num_classes + 1
        hip.gather_rows(pl.cls, pl.sub_pos, pl.sub_cls, B, Q, R, nc)
        hip.gather_rows(pl.cls, pl.obj_pos, pl.obj_cls, B, Q, R, nc)
        if not self._fused_pair_masks():
            self._gather_segs(pl)

    def _gather_segs(self, pl):
        B, Q, R = pl.B, self.num_obj_query, self.num_rel_query
        hip.gather_rows(pl.MP, pl.sub_pos, pl.sub_seg, B, Q, R, pl.HW2)
        hip.gather_rows(pl.MP, pl.obj_pos, pl.obj_seg, B, Q, R, pl.HW2)

    def _outputs(self, pl):
        B, Q, R = pl.B, self.num_obj_query, self.num_rel_query
        H2, W2 = pl.hw2
        return (dict(sub=pl.sub_cls, obj=pl.obj_cls, cls=pl.cls, rel=pl.rel, importance=pl.imp),
                dict(mask=pl.MP.view(B, Q, H2, W2), sub_seg=pl.sub_seg.view(B, R, H2, W2),
                     obj_seg=pl.obj_seg.view(B, R, H2, W2)))

    def _check_feats(self, feats, img_metas):
        pv = getattr(self, "_packed_version", None)
        if self.w is not None and pv is not None and pv != self._weights_version():
            self._drop_weight_state()          # a parameter was updated in place
        B = len(img_metas)
        assert len(feats) == 4 and all(f.shape[0] == B for f in feats)
        nchw = all(f.is_contiguous() for f in feats)
        nhwc = not nchw and all(f.is_contiguous(memory_format=torch.channels_last) for f in feats)
        for f, c in zip(feats, self.in_channels):
            if not f.is_cuda or f.dtype != torch.float32 or f.shape[1] != c or not (nchw or nhwc):
                raise RuntimeError("feats must be fp32 [B,C,H,W] device tensors with channels %s, "
                                   "all contiguous or all in channels_last memory format"
                                   % self.in_channels)
        if self.device is None:
            self.to(feats[0].device)
        shapes = [tuple(feats[3 - l].shape[-2:]) for l in range(3)]
        self._feats_nhwc = nhwc
        return B, shapes, tuple(feats[0].shape[-2:])

    def _run_stage(self, which, pl, feats=None):
        """Run stage 'a' or 'b' of plan `pl` on the current stream: eagerly, or (with
        `use_graphs`) as one hipGraph replay.  A stage is captured once it has run
        `graph_after` times eagerly -- without any host synchronisation: nothing allocates,
        every buffer is a view of the slot's arena (plans.py)."""
        cfg = (self.exact_mask_order, self.conv_algo, self.fuse_ppn_front, self.grid_reserve,
               tuple(self.enc_fused_ln), self.group_input_convs,
               getattr(self, "fuse_mask_pack", True), self.gemm_arithmetic, self.msda_s3_out,
               self._fused_pair_masks(), bool(getattr(self, "fuse_encoder_ffn", 0)),
               bool(getattr(self, "enc_proj_reads_rows", 0)),
               getattr(self, "gather_mask_stencil", True), getattr(self, "fuse_lateral_upadd", False))
        if pl.graph_cfg != cfg:          # a captured graph bakes these switches in
            pl.graph_a = pl.graph_b = None
            pl.graphs_a = OrderedDict()
            pl.graph_c = PlanCache(self.POST_VIEWS)
            pl.graph_cfg = cfg
        cur = torch.cuda.current_stream(self.device)
        pl.streams[cur.cuda_stream] = cur
        try:
            self._run_stage_on(which, pl, feats, cur)
        finally:
            plans.note_use(cur)

    def _run_stage_on(self, which, pl, feats, cur):
        if which == "a":
            if not pl.pe_waited:
                # the position tables are shared by the slots and filled on the stream that
                # first saw the shape: order this stream behind them (until they are done)
                if pl.pe_ready.query():
                    pl.pe_waited = True
                else:
                    cur.wait_event(pl.pe_ready)
            ptrs = tuple(f.data_ptr() for f in feats)
            # A stage-A graph is tied to the caller's feature buffers (captured on them: no
            # staging copy).  One plan can meet several buffer sets -- image sizes that differ
            # by a pixel share a feature pyramid, hence this plan, but not the backbone's
            # buffers -- so up to STAGE_A_GRAPHS graphs are kept per plan, by pointer; a
            # caller that hands over new buffers every time is simply served eagerly.
            ent = pl.graphs_a.get(ptrs)
            if ent is None:
                if len(pl.graphs_a) >= self.STAGE_A_GRAPHS:     # forget the oldest entry that
                    for k, e in pl.graphs_a.items():            # never got as far as a graph
                        if e["graph"] is None:
                            del pl.graphs_a[k]
                            break
                    else:
                        # every entry owns a graph: the least recently used one goes (at a quiet
                        # point: its graph may still be replaying otherwise).  Its `feats` are what
                        # kept a producer's OLD buffers alive -- e.g. the backbone's arena of
                        # before a growth, hundreds of MB that nothing would ever read again
                        # 
                        if plans.quiet(cur):
                            torch.cuda.current_stream(self.device).synchronize()
                            pl.graphs_a.popitem(last=False)
                if len(pl.graphs_a) < self.STAGE_A_GRAPHS:
                    ent = pl.graphs_a[ptrs] = dict(calls=0, graph=None, feats=None)
            else:
                pl.graphs_a.move_to_end(ptrs)
            if self.use_graphs and ent is not None and ent["graph"] is None \
                    and ent["calls"] >= self.graph_after and plans.quiet(cur):
                ent["feats"] = list(feats)
                self._note_capture(pl, ("a", ptrs))
                ent["graph"] = self._capture(lambda: self._stage_a(ent["feats"], pl))
            if ent is not None:
                ent["calls"] += 1
            pl.calls_a += 1
            graph = ent["graph"] if (self.use_graphs and ent is not None) else None
            pl.graph_a, pl.static_ptrs = graph, (ptrs if graph is not None else None)
            if pl.feats_read is None:
                pl.feats_read = torch.cuda.Event()
            if graph is not None:
                graph.replay()
            else:
                self._stage_a(feats, pl)
            pl.feats_read.record()      # the caller's feature buffers are free again
        else:
            if self.use_graphs and pl.graph_b is None and pl.calls_b >= self.graph_after \
                    and plans.quiet(cur):
                self._note_capture(pl, "b")
                pl.graph_b = self._capture(lambda: self._stage_b(pl))
            pl.calls_b += 1
            if self.use_graphs and pl.graph_b is not None:
                pl.graph_b.replay()
            else:
                self._stage_b(pl)

    def _note_capture(self, pl, stage):
        """Bookkeeping for the bench / tests: a capture of a (plan key, stage) that had been
        captured before in this head's life is a RE-capture (the plan was evicted, its arena
        grew, the weights or the caller's buffers changed)."""
        seen = self.__dict__.setdefault("_captured", set())
        if len(seen) > 8192:          # (bookkeeping only: never let it grow with a long run)
            seen.clear()
        k = (pl.key, stage)
        if k in seen:
            self.recaptures = getattr(self, "recaptures", 0) + 1
        seen.add(k)

    _capture_streams = {}
    captures = 0          # graphs captured so far in this process (a counter for the bench / tests)

    @staticmethod
    def _capture(fn):
        """Record `fn`'s launches into a hipGraph, on a private stream.  Callers capture at quiet
        points only (`plans.quiet`, see there for the measurement behind it); the device wait in
        front makes that robust against streams this package does not know.  Unlike
        `torch.cuda.graph()` no garbage collection / allocator trim: the launches allocate
        nothing (arena views).  thread_local: other threads (the RCCL watchdog, the result
        streamer's worker) may touch the runtime while this thread captures."""
        torch.cuda.synchronize()
        dev = torch.cuda.current_device()
        cs = CrossHead2._capture_streams.get(dev)
        if cs is None:
            cs = CrossHead2._capture_streams[dev] = torch.cuda.Stream(dev)
        g = torch.cuda.CUDAGraph()
        # No cyclic garbage collection while the stream is capturing: a collection that happens to
        # run now would destroy whatever unreachable hipGraphs / events / device tensors the
        # PROCESS has lying around (another, dropped detector's plans are such a cycle) from inside
        # the capture, and a runtime call that is not allowed there ends in abort() -- seen in the
        # test suite once it had grown enough garbage in front of a capture (round 6).
        # torch.cuda.graph() collects up front for the same reason; deferring costs nothing.
        import gc
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(cs):
                g.capture_begin(capture_error_mode="thread_local")
                try:
                    fn()
                except BaseException as first:
                    # end the capture so that the stream leaves capture mode, but report what
                    # went wrong inside it (a refused launch, a shape error), not the invalidated
                    # capture
                    try:
                        g.capture_end()
                    except Exception:
                        pass
                    raise first
                g.capture_end()
        finally:
            if gc_was_on:
                gc.enable()
        CrossHead2.captures += 1          # (counted once it exists)
        return g

    @torch.no_grad()
    @hip.on_device
    def forward(self, feats, img_metas, slot=0):
        """feats: [C2, C3, C4, C5] NCHW fp32 on the GPU; returns the reference's two
        dicts (pairnet_head.py:405-417).  Output tensors are views of per-shape
        buffers that the next forward() of the same shape (and slot) overwrites."""
        pl = self._forward_plan(feats, img_metas, slot)
        if self._fused_pair_masks():
            # stage B left sub_seg / obj_seg alone (post-processing does not read them): the
            # caller of forward() may, so they are gathered here, outside the stage's graph
            self._gather_segs(pl)
        return self._outputs(pl)

    __call__ = forward

    @torch.no_grad()
    @hip.on_device
    def _forward_plan(self, feats, img_metas, slot=0):
        """Both stages on the plan of this shape; returns the plan."""
        B, shapes, hw2 = self._check_feats(feats, img_metas)
        pl = self._plan(B, shapes, hw2, slot, self._feats_nhwc)
        self._run_stage("a", pl, feats)
        self._run_stage("b", pl)
        self._last_plan = pl
        return pl

    @torch.no_grad()
    @hip.on_device
    def forward_head(self, decoder_out, mask_feature, attn_mask_target_size):
        """Reference signature (pairnet_head.py:216): decoder_out (Q, B, C) seq-first,
        mask_feature (B, C, h, w); returns cls_pred (B,Q,nc), mask_pred (B,Q,h,w),
        attn_mask (B*heads, Q, th*tw) bool."""
        if self.w is None:
            if self.device is None:
                self.to(decoder_out.device)
            self._pack()
        w = self.w
        Q, B, _ = decoder_out.shape
        h, wd = mask_feature.shape[-2:]
        th, tw = attn_mask_target_size
        dev, f32 = self.device, torch.float32
        E = lambda *s: torch.empty(*s, device=dev, dtype=f32)
        q = decoder_out.permute(1, 0, 2).contiguous().view(B * Q, 256)
        mf = mask_feature.permute(0, 2, 3, 1).contiguous().view(B, h * wd, 256)
        qn, m1, m2, me = E(B * Q, 256), E(B * Q, 256), E(B * Q, 256), E(B * Q, 256)
        cls = E(B, Q, self.num_classes + 1)
        mp, ml = E(B, Q, h * wd), E(B * Q, th * tw)
        hip.layernorm(q, w["transformer_decoder.post_norm.weight"],
                      w["transformer_decoder.post_norm.bias"], qn)
        hip.linear(qn, w["cls_embed.weight"], w["cls_embed.bias"], cls.view(B * Q, -1))
        hip.linear(qn, w["mask_embed.0.weight"], w["mask_embed.0.bias"], m1, relu=True)
        hip.linear(m1, w["mask_embed.2.weight"], w["mask_embed.2.bias"], m2, relu=True)
        hip.linear(m2, w["mask_embed.4.weight"], w["mask_embed.4.bias"], me)
        hip.gemm(me, mf, mp, M=Q, N=h * wd, K=256, lda=256, ldw=256, ldc=h * wd, batch=B,
                 sA=Q * 256, sW=h * wd * 256, sC=Q * h * wd)
        hip.bilinear_planar(mp, ml, B * Q, h, wd, th, tw)
        attn = (ml.view(B, 1, Q, th * tw) < 0).expand(B, self.n_heads, Q, th * tw)
        return cls, mp.view(B, Q, h, wd), attn.reshape(B * self.n_heads, Q, th * tw)

    # ------------------------------------------------------- post-processing
    class ResultList(list):
        """The list `get_bboxes` returns, plus the device-side panoptic loop states of its
        images (`panoptic_status` reads them at the caller's D2H point)."""
        panoptic_jobs = ()

    def _post_buffers(self, anchor, key, build):
        """Post-processing buffers for FOREIGN inputs (tensors that are not a plan's own
        outputs), per (input buffer, output size): a small bounded table, oldest entry
        dropped first.  The head's own outputs -- the hot loop -- take views of the slot's
        post-processing arena instead (`_post_views`)."""
        k = (anchor.data_ptr(), str(anchor.device)) + tuple(key)
        table = self._post
        pb = table.get(k)
        if pb is None:
            if len(table) >= self.POST_ENTRIES:
                # rare and not on the steady-state path: wait for the device first (queued
                # kernels may still reference the entry's buffers)
                torch.cuda.synchronize(anchor.device)
                table.pop(next(iter(table)))
            pb = table[k] = build()
        return pb

    def _post_layout(self, E, sizes):
        """Post-processing buffers of one batch, `sizes` = [(H0, W0)] per image."""
        R, Q = self.num_rel_query, self.num_obj_query
        out = []
        for H0, W0 in sizes:
            out.append(dict(
                labels=E.i64(2 * R), sc_tmp=E(2 * R), r_dists=E(R, self.num_relations + 1),
                masks=E.u8(2 * R, H0, W0), all_labels=E.i64(Q), all_scores=E(Q),
                state=E.u8(hip.panoptic_state_bytes()), up=E(Q, H0 * W0), area=E.i32(256),
                seg=E.i64(H0 * W0)))
        return out

    def _post_views(self, pl, sizes):
        """Views of slot `pl.slot`'s post-processing arena for a batch whose images have the
        original sizes `sizes`: like the plans themselves, no allocation per (shape, size) --
        a keep-ratio evaluation set has about as many original sizes as images."""
        sizes = tuple(sizes)
        pv = pl.post_views.get(sizes)
        if pv is not None:
            pl.post_views.move_to_end(sizes)
            return pv
        # buffer sizes depend on the pixel COUNT only: the arena's envelope is (images,
        # pixels of the largest image)
        dims = (len(sizes), max(h * w for h, w in sizes))
        pv = self._post_arena(pl.slot).carve(
            lambda E: self._post_layout(E, sizes), dims,
            lambda d: measure_bytes(lambda E: self._post_layout(E, [(1, d[1])] * d[0])))
        pl.post_views[sizes] = pv
        while len(pl.post_views) > self.POST_VIEWS:
            pl.post_views.popitem(last=False)     # (views: nothing to free, nothing to wait for)
        return pv

    class _PostGraph:
        def __init__(self, pl):
            self.pl, self.calls, self.graph, self.res = pl, 0, None, None

        def busy_events(self):
            return self.pl.busy_events() if self.graph is not None else []

    def _own_plan(self, cls_scores, mask_preds):
        """The plan whose outputs these dicts are (None for foreign tensors)."""
        pl = getattr(self, "_last_plan", None)
        if pl is not None and "cls" in cls_scores and "mask" in mask_preds \
                and cls_scores["cls"].data_ptr() == pl.cls.data_ptr() \
                and mask_preds["mask"].data_ptr() == pl.MP.data_ptr():
            return pl
        return None

    @torch.no_grad()
    @hip.on_device
    def get_bboxes(self, cls_scores, mask_preds, img_metas, rescale=False):
        """pairnet_head.py:760-786.  With `use_graphs`, the post-processing of a plan's own
        outputs is replayed as one hipGraph per (plan, image sizes), captured like the stage
        graphs after `graph_after` eager calls."""
        pl = self._own_plan(cls_scores, mask_preds)
        if pl is None or not self.use_graphs:
            return self._get_bboxes_all(cls_scores, mask_preds, img_metas, rescale, pl)
        cur = torch.cuda.current_stream(self.device)
        pl.streams[cur.cuda_stream] = cur
        key = (tuple((tuple(m["img_shape"]), tuple(float(v) for v in m["scale_factor"]))
                     for m in img_metas), bool(rescale))
        ent = pl.graph_c.get(key)
        if ent is None:
            ent = pl.graph_c[key] = CrossHead2._PostGraph(pl)
        if ent.graph is None:
            if ent.calls < self.graph_after or not plans.quiet(cur):
                ent.calls += 1
                res = self._get_bboxes_all(cls_scores, mask_preds, img_metas, rescale, pl)
                plans.note_use(cur)
                return res
            self._post_views(pl, self._orig_sizes(img_metas))   # (made / grown outside the capture)
            pl.graph_c[key] = ent
            box = {}
            ent.graph = self._capture(lambda: box.update(
                res=self._get_bboxes_all(cls_scores, mask_preds, img_metas, rescale, pl)))
            ent.res = box["res"]
        ent.graph.replay()
        plans.note_use(cur)
        self._pan_jobs = list(ent.res.panoptic_jobs)
        return ent.res

    @staticmethod
    def _orig_sizes(img_metas):
        return [(round(m["img_shape"][0] / m["scale_factor"][1]),
                 round(m["img_shape"][1] / m["scale_factor"][0])) for m in img_metas]

    def _get_bboxes_all(self, cls_scores, mask_preds, img_metas, rescale, pl=None):
        self._pan_jobs = []
        pv = self._post_views(pl, self._orig_sizes(img_metas)) if pl is not None else None
        res = CrossHead2.ResultList(self._get_bboxes_single(
            mask_preds["mask"][i], cls_scores["cls"][i], cls_scores["sub"][i],
            cls_scores["obj"][i], cls_scores["rel"][i], mask_preds["sub_seg"][i],
            mask_preds["obj_seg"][i], img_metas[i]["img_shape"],
            img_metas[i]["scale_factor"], rescale, pb=pv[i] if pv is not None else None,
            own=(pl, i) if pl is not None else None)
            for i in range(len(img_metas)))
        res.panoptic_jobs = tuple(self._pan_jobs)
        return res

    def _get_bboxes_single(self, all_masks, all_cls, s_cls, o_cls, r_cls, s_seg, o_seg,
                           img_shape, scale_factor, rescale=False, pb=None, own=None):
        """pairnet_head.py:788-924 on the device, without any host round trip (every
        launch is asynchronous; `panoptic_status()` reads the loop flags back at the
        caller's D2H point).  The outputs are views of buffers owned by the head -- for the
        head's own outputs views of the slot's post-processing arena (`pb`), for foreign
        inputs one set per (input buffer, output size): the next call overwrites them.
        `own` = (plan, image) when the inputs are that plan's outputs: with `fused_pair_masks`
        the result masks then come from the plan's MP / sub_pos / obj_pos and `s_seg` / `o_seg`
        are not read."""
        assert len(s_cls) == len(o_cls) == len(r_cls)
        dev = all_cls.device
        R, Q = self.num_rel_query, all_cls.shape[0]
        nc = all_cls.shape[-1]
        H0 = round(img_shape[0] / scale_factor[1])
        W0 = round(img_shape[1] / scale_factor[0])
        h, wd = all_masks.shape[-2:]
        for t in (all_masks, all_cls, s_cls, o_cls, r_cls, s_seg, o_seg):
            if not t.is_contiguous():
                raise RuntimeError("get_bboxes takes contiguous tensors (the head's own outputs)")

        def build():
            i64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int64)
            f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
            return dict(labels=i64(2 * R), sc_tmp=f32(2 * R), r_dists=f32(R, self.num_relations + 1),
                        masks=torch.empty(2 * R, H0, W0, device=dev, dtype=torch.uint8),
                        all_labels=i64(Q), all_scores=f32(Q),
                        state=torch.empty(hip.panoptic_state_bytes(), device=dev, dtype=torch.uint8),
                        up=f32(Q, H0 * W0), area=torch.empty(256, device=dev, dtype=torch.int32),
                        seg=i64(H0 * W0))
        if pb is None:
            pb = self._post_buffers(all_cls, (H0, W0, Q, R), build)
        # triplet labels (1-based) and relation distributions (:811-820)
        labels = pb["labels"]
        hip.cls_argmax(s_cls, labels[:R], pb["sc_tmp"][:R], R, nc, 1)
        hip.cls_argmax(o_cls, labels[R:], pb["sc_tmp"][R:], R, nc, 1)
        hip.rel_dists(r_cls, pb["r_dists"], R, self.num_relations)
        # subject / object masks at the original image size (:826-843)
        masks_u8 = pb["masks"]
        if own is not None and self._fused_pair_masks():
            pl, i = own
            hip.pair_masks(pl.MP[i], pl.sub_pos[i], pl.obj_pos[i], masks_u8, Q, R, h, wd, H0, W0)
        else:
            hip.bilinear_planar_gt0(s_seg, masks_u8[:R], R, h, wd, H0, W0)
            hip.bilinear_planar_gt0(o_seg, masks_u8[R:], R, h, wd, H0, W0)
        # panoptic map (:823-825, :845-905), entirely on the device: keep list, stuff-class
        # merging, argmax and the "drop segments of area <= 4 and redo" loop are enqueued as
        # a bounded number of rounds (csrc/postproc.hip); whether the loop has converged is
        # a flag the caller reads at its D2H point (`panoptic_status`).  pan_img stays on the
        # device (the reference returns a host tensor, :883): a fresh multi-MB host
        # allocation per image is an mmap/munmap pair, and on ROCm every munmap runs the
        # amdgpu MMU notifier against the busy GPU (~75 ms stalls measured).
        hip.cls_argmax(all_cls, pb["all_labels"], pb["all_scores"], Q, nc)
        hip.panoptic_device(all_masks, pb["all_labels"], pb["all_scores"], Q, nc - 1, h, wd, H0,
                            W0, pb["state"], pb["up"], pb["area"], pb["seg"])
        self._pan_jobs.append((pb["state"], pb["up"], pb["area"], pb["seg"], H0, W0))
        # the reference's dummy outputs (:907-913) are constants: made once per device
        key = (str(dev), R)
        if key not in self._dummies:
            self._dummies[key] = (torch.zeros((2 * R, 5), device=dev), torch.zeros(R, device=dev),
                                  torch.zeros(R, device=dev),
                                  torch.arange(2 * R, dtype=torch.int).reshape(2, -1).T)
        det_bboxes, r_scores, r_labels, rel_pairs = self._dummies[key]
        return (det_bboxes, labels, rel_pairs, masks_u8.view(torch.bool),
                pb["seg"].view(H0, W0), r_scores, r_labels, pb["r_dists"])

    def panoptic_status(self, results=None):
        """Finish and check the panoptic loops of `results` (a list `get_bboxes` returned;
        default: the last one).  The reference loops on the host until no segment of area
        <= 4 is left (pairnet_head.py:893-905) and fails with an IndexError when every
        segment is filtered (:882).  The device loop runs hip.PAN_ROUNDS rounds up front;
        here -- one small D2H per image, at a point where the caller copies results to the
        host anyway -- unfinished loops are continued to convergence and the IndexError is
        raised.  Returns one dict(nkeep, rounds) per image."""
        jobs = self._pan_jobs if results is None else results.panoptic_jobs
        out = []
        for state, up, area, seg, H0, W0 in jobs:
            while True:
                nkeep, active, rounds, all_gone = state[:16].cpu().view(torch.int32).tolist()
                if all_gone:
                    raise IndexError("every panoptic segment was filtered (the reference fails "
                                     "here too, pairnet_head.py:882)")
                if not active:
                    break
                with torch.cuda.device(state.device):
                    hip.panoptic_continue(state, up, area, seg, H0, W0)
            out.append(dict(nkeep=nkeep, rounds=rounds))
        return out

    def loss_object(self):
        """The `CrossHead2Loss` behind `loss` (built on first use; it owns SeesawLoss's persistent
        `cum_samples`, which a checkpoint of a training run carries)."""
        if self._loss is None:
            from .losses import CrossHead2Loss
            self._loss = CrossHead2Loss(self.num_classes, self.num_relations, self.num_obj_query,
                                        self.num_rel_query, **self._loss_cfg)
        return self._loss

    def loss(self, all_cls_scores, all_mask_preds, gt_rels_list, gt_bboxes_list, gt_labels_list,
             gt_masks_list, img_metas, gt_bboxes_ignore=None, **kw):
        """The reference's `CrossHead2.loss` (pairnet_head.py:419-477), forward values only:
        {loss_r_cls, loss_sub_cls, loss_obj_cls, loss_match} as 0-dim device tensors, from the
        two dicts `forward` returns and the per-image ground truth (losses.py; `point_coords=`
        fixes the sampled mask points, default torch.rand like the reference)."""
        return self.loss_object().loss(all_cls_scores, all_mask_preds, gt_rels_list, gt_bboxes_list,
                               gt_labels_list, gt_masks_list, img_metas,
                               gt_bboxes_ignore=gt_bboxes_ignore, **kw)

    def forward_train(self, *a, **kw):
        raise NotImplementedError(
            "forward_train + autograd is not how this head trains: `val_losses()` / `loss()` give the "
            "reference's loss values, `loss(..., grads={})` their gradients w.r.t. the logits, and "
            "`pairnet_amd.TailTrainer(head).step(...)` runs one iteration (loss -> backward through "
            "the head, optionally the backbone -> clip -> AdamW)")

    def val_losses(self, x, img_metas, gt_rels, gt_bboxes, gt_labels=None, gt_masks=None,
                   gt_bboxes_ignore=None, **kw):
        """The values of the reference's `forward_train` (pairnet_head.py:720-757):
        `outs = self(x, img_metas)`, then `loss(*outs, gt_rels, gt_bboxes, gt_labels, gt_masks,
        img_metas)`.  Forward only."""
        if gt_labels is None:
            raise ValueError("gt_labels is required (the reference's four-argument form feeds "
                             "loss() one positional argument short)")
        outs = self.forward(x, img_metas)
        return self.loss(*outs, gt_rels, gt_bboxes, gt_labels, gt_masks, img_metas,
                         gt_bboxes_ignore=gt_bboxes_ignore, **kw)

    def pair_positions(self, pl=None):
        """(sub_pos, obj_pos): per image the query rows of the R selected pairs
        (pairnet_head.py:338-340) of plan `pl` (default: the last forward's) -- what the
        distributed test loop packs into the triplet records next to labels and r_dists."""
        pl = pl if pl is not None else self._last_plan
        return pl.sub_pos, pl.obj_pos

    def simple_test_bboxes(self, feats, img_metas, rescale=False):
        """pairnet_head.py:926-930."""
        if not self._fused_pair_masks():
            return self.get_bboxes(*self.forward(feats, img_metas), img_metas, rescale=rescale)
        # (the post-processing of the head's own outputs does not read sub_seg / obj_seg: no
        # gathers of them on this path)
        pl = self._forward_plan(feats, img_metas)
        return self.get_bboxes(*self._outputs(pl), img_metas, rescale=rescale)

    def simple_test(self, feats, img_metas, rescale=False):
        return self.simple_test_bboxes(feats, img_metas, rescale=rescale)
