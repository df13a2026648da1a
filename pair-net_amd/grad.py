"""Backward of Pair-Net's own tail on the MI355X (second slice; no optimizer, no
DDP): given the object decoder's output queries `q` and the gradients of the four loss terms
with respect to the head's logits (`CrossHead2.loss(..., grads={})`, csrc/loss.hip), the
gradients of everything between them --

  * the Relation Fusion decoder x6 + `rel_cls_embed` (pairnet_head.py:353-378; post-norm layers
    in the order cross-attention, norm, self-attention, norm, FFN, norm: facebook_detr.py:378-432),
  * the pair-feature gather (:342-351) back onto the query rows,
  * the Pair Proposal Network: `sub_query_update` / `obj_query_update` MLPs, F.normalize, the
    cosine matrix (:322-333) and the Matrix Learner ConvTiny (frameworks/cnn_factory.py:6-53),
  * optionally the subject / object class gathers (:380-390) through `cls_embed` and `post_norm`
    (:236-238) -- the reference DETACHES `cls_pred` there, so by default they carry no gradient

-- with respect to `q` and to every parameter on the way, named and laid out as the reference's
state dict.  In the reference this is `torch.autograd` behind `losses.backward()`; here the
forward is re-run with the product's forward kernels into a tape of per-layer buffers
(`forward`), and `backward` walks it with csrc/grad.hip's kernels plus `pn_gemm_f32` (a linear
layer's dX = dY W and dW = dY^T X are GEMMs on transposed operands) and `pn_conv2d_nhwc_ex_f32`
(the 64 -> 64 convolution's data gradient).  The top-k pair selection is piecewise constant: the
selected (subject, object) rows are inputs of the backward pass, exactly as autograd treats them.

`HeadGrad` puts the nine masked decoder layers in front of that tail, `BBoxTailGrad` is the tail
under `CrossHeadBBox`.  What all tapes share (the flat gradient layout, the linear / LayerNorm
steps) is `Tape` (tape.py); the pixel decoder's tape is in pixel_grad.py, the backbones' in
backbone_grad.py, the tapes behind the segmentation losses (the mask branch) in seg_grad.py.

Checked against autograd through the reference-pinned oracle (tests/test_grad_gpu.py: 1e-4
relative on `reldec.npz`, `ppn_sep.npz` and the queries of an 800x1333 image).
"""
import math
from collections import OrderedDict, namedtuple

import torch

from . import hip
from .tape import Tape
# (api.py takes every tape's public name from here, as it always has; they live in their own files)
from .pixel_grad import PixelDecoderGrad  # noqa: F401
from .backbone_grad import BackboneGrad, SwinBackboneGrad, SwinStagesGrad  # noqa: F401

__all__ = ["RelationTailGrad", "HeadGrad", "PixelDecoderGrad", "BackboneGrad", "SwinBackboneGrad",
           "SwinStagesGrad", "FfnDropout", "BBoxTailGrad"]


class FfnDropout(namedtuple("FfnDropout", "p seed subseq step layer")):
    """Descriptor of the Relation Fusion decoder's training-mode FFN dropout (mmcv FFN.layers: two
    `nn.Dropout(ffn_drop)` per layer; configs/mask2former/pairnet.py:121-129): rate `p`, and the
    counter the keep bits are a function of (csrc/dropout.hip) -- `seed`, `subseq` (the
    data-parallel rank), `step` (the iteration), `layer` (filled in per layer by the tape).  Site
    2 * layer + 0 is the hidden rows [B * R, ffn] after the ReLU, 2 * layer + 1 the FFN's output
    [B * R, 256] before the shortcut; the element index is the position in the contiguous
    batch-major buffer.  The backward pass passes the same descriptor: nothing is stored."""
    __slots__ = ()

    def __new__(cls, p, seed=0, subseq=0, step=0, layer=0):
        p = float(p)
        if not 0.0 <= p < 1.0:
            raise ValueError("dropout rate %r outside [0, 1)" % p)
        return super().__new__(cls, p, int(seed), int(subseq), int(step), int(layer))

    def apply(self, x, out, which, res=None):
        """out = drop(x) (+ res) at this layer's site `which` (0: hidden rows, 1: FFN output)."""
        hip.dropout(x, out, self.p, self.seed, self.subseq, self.step, 2 * self.layer + which,
                    res=res)

    def keep(self, n, which, device=None):
        """The site's keep bits for n elements (uint8 device tensor; for tests and oracles)."""
        return hip.dropout_keep(n, self.p, self.seed, self.subseq, self.step,
                                2 * self.layer + which, device=device)


class RelationTailGrad(Tape):
    """tape = RelationTailGrad(head); out = tape.forward(q); dq, grads = tape.backward(...)

    `q`: [B * Q, 256] fp32 on the head's device, batch-major (a plan's `pl.q`: the last
    masked-decoder layer's output BEFORE `post_norm`).  `forward` returns dict(rel [B, R, C],
    importance [B, Q, Q], importance_raw, sub / obj [B, R, nc], cls [B, Q, nc], sub_pos,
    obj_pos); the pair list is the top-k of `importance` unless `sub_pos` / `obj_pos` [B, R]
    int64 are given.  `backward(g_rel, g_importance, g_sub, g_obj, cls_detached=True)` (any subset;
    shapes of the outputs) returns (dq [B * Q, 256], {reference parameter name: gradient}).
    """

    def __init__(self, head, flat=None, base=0):
        super().__init__(head, flat, base)
        self.head = head
        self.Q, self.R = head.num_obj_query, head.num_rel_query
        self.L = head.num_rel_layers
        self.ffn = head.rel_ffn
        self.scale = 1.0 / math.sqrt(32.0)

    @staticmethod
    def param_groups(head):
        """[(group, [reference parameter names])] in the order backward() completes them."""
        L = head.num_rel_layers
        groups = [("rel_cls_embed", ["rel_cls_embed.weight", "rel_cls_embed.bias"])]
        for i in reversed(range(L)):
            groups.append(("relation_decoder.layers.%d" % i,
                           RelationTailGrad._layer_names("relation_decoder.layers.%d." % i)))
        groups.append(("rel_query", ["rel_query_feat.weight", "rel_query_embed.weight",
                                     "rel_query_embed2.weight"]))
        ml = "update_importance.conv_layers."
        groups.append(("update_importance", [ml + "%d.0.%s" % (j, n) for j in (2, 1, 0)
                                             for n in ("weight", "bias")]))
        for side in ("sub", "obj"):
            groups.append((side + "_query_update", ["%s_query_update.%d.%s" % (side, j, n)
                                                    for j in (4, 2, 0) for n in ("weight", "bias")]))
        groups.append(RelationTailGrad.CLS_GROUP)
        return groups

    CLS_GROUP = ("cls", ["cls_embed.weight", "cls_embed.bias", "transformer_decoder.post_norm.weight",
                         "transformer_decoder.post_norm.bias"])

    @staticmethod
    def _layer_names(pre):
        names = []
        for a in ("attentions.0.attn.", "attentions.1.attn."):
            names += [pre + a + n for n in ("in_proj_weight", "in_proj_bias", "out_proj.weight",
                                            "out_proj.bias")]
        names += [pre + "norms.%d.%s" % (j, n) for j in range(3) for n in ("weight", "bias")]
        names += [pre + "ffns.0.layers.0.0.weight", pre + "ffns.0.layers.0.0.bias",
                  pre + "ffns.0.layers.1.weight", pre + "ffns.0.layers.1.bias"]
        return names

    # ------------------------------------------------------------------ forward with a tape
    @torch.no_grad()
    @hip.on_device
    def forward(self, q, sub_pos=None, obj_pos=None, dropout=None):
        """`dropout` (an `FfnDropout`, default None): run the Relation Fusion decoder in the
        reference's train mode; nothing else of the tail has a non-zero rate.  `self.t["rel"]` keeps
        the returned relation logits."""
        head, w, E, Q = self.head, self.head.w, self._E, self.Q
        if not (q.is_cuda and q.dtype == torch.float32 and q.dim() == 2 and q.shape[1] == 256
                and q.is_contiguous() and q.shape[0] % Q == 0):
            raise RuntimeError("q must be a contiguous [B * Q, 256] fp32 device tensor")
        B = q.shape[0] // Q
        t = self.t = dict(B=B, q=q)
        # ---- post_norm + cls_embed (pairnet_head.py:236-238) ----
        nc = head.num_classes + 1
        t["qn"] = E(B * Q, 256)
        hip.layernorm(q, w["transformer_decoder.post_norm.weight"],
                      w["transformer_decoder.post_norm.bias"], t["qn"])
        cls = E(B, Q, nc)
        hip.linear(t["qn"], w["cls_embed.weight"], w["cls_embed.bias"], cls.view(B * Q, nc))
        # ---- Pair Proposal Network (:322-340), pair features (:342-351), relation decoder ----
        imp, raw, sub_pos, obj_pos = self._ppn_forward(q, B, sub_pos, obj_pos)
        return self._pairs_forward(q, cls, imp, raw, sub_pos, obj_pos, dropout)

    def _ppn_forward(self, q, B, sub_pos, obj_pos):
        """The Pair Proposal Network (pairnet_head.py:322-340) on the query rows q, into the tape
        `self.t`: the two MLPs, the cosine matrix, the Matrix Learner, then the pair list -- the
        top-k of the importance matrix unless `sub_pos` / `obj_pos` are given.
        -> (importance, importance_raw, sub_pos, obj_pos)."""
        w, E, t = self.head.w, self._E, self.t
        Q, R = self.Q, self.R
        for side in ("sub", "obj"):
            mlp = side + "_query_update"
            h1, h2, e = E(B * Q, 256), E(B * Q, 256), E(B * Q, 256)
            hip.linear(q, w[mlp + ".0.weight"], w[mlp + ".0.bias"], h1, relu=True)
            hip.linear(h1, w[mlp + ".2.weight"], w[mlp + ".2.bias"], h2, relu=True)
            hip.linear(h2, w[mlp + ".4.weight"], w[mlp + ".4.bias"], e)
            t[side] = (h1, h2, e)
        ml = "update_importance.conv_layers."
        raw, c1, c2, imp = E(B, Q, Q), E(B, Q, Q, 64), E(B, Q, Q, 64), E(B, Q, Q)
        hip.ppn_front(t["sub"][2], t["obj"][2], w[ml + "0.0.weight"], w[ml + "0.0.bias"], raw, c1,
                      B, Q)
        hip.conv2d_ex(c1, w[ml + "1.0.weight"], w[ml + "1.0.bias"], None, c2, B, Q, Q, 64, 64, 7,
                      7, 1, 3, relu=True)
        hip.mlearner_last(c2, w[ml + "2.0.weight"], w[ml + "2.0.bias"], imp, B, Q)
        t.update(raw=raw, c1=c1, c2=c2)
        i64 = lambda *s: torch.empty(*s, device=self.dev, dtype=torch.int64)
        pair_idx = i64(B, 2 * R)
        if sub_pos is None:
            topk, sub_pos, obj_pos = i64(B, R), i64(B, R), i64(B, R)
            hip.topk_pairs(imp, topk, sub_pos, obj_pos, B, Q, R, pair=pair_idx)
        else:
            sub_pos = sub_pos.to(self.dev, torch.int64).contiguous()
            obj_pos = obj_pos.to(self.dev, torch.int64).contiguous()
            pair_idx[:, :R].copy_(sub_pos)
            pair_idx[:, R:].copy_(obj_pos)
        t.update(sub_pos=sub_pos, obj_pos=obj_pos, pair_idx=pair_idx)
        return imp, raw, sub_pos, obj_pos

    def _pairs_forward(self, q, cls, imp, raw, sub_pos, obj_pos, dropout):
        """The pair features (:342-351) through the relation decoder, and the subject / object
        class logits gathered from `cls` [B, Q, nc]; -> forward()'s dict."""
        E, t = self._E, self.t
        B, Q, R, nc = t["B"], self.Q, self.R, cls.shape[2]
        pair = E(B * 2 * R, 256)
        hip.gather_rows(q, t["pair_idx"], pair, B, Q, 2 * R, 256)
        rel = self._relation_forward(pair, B, dropout)
        sub, obj = E(B, R, nc), E(B, R, nc)
        hip.gather_rows(cls, sub_pos, sub, B, Q, R, nc)
        hip.gather_rows(cls, obj_pos, obj, B, Q, R, nc)
        return dict(rel=rel, importance=imp, importance_raw=raw, sub=sub, obj=obj, cls=cls,
                    sub_pos=sub_pos, obj_pos=obj_pos)

    def _layer_fwd(self, pre, x, qpos, K, V, B, nq, nk, ffn, scr, bits=None, rowall=None,
                   drop=None):
        """One post-norm decoder layer (facebook_detr.py:378-432; order cross-attention, norm,
        self-attention, norm, FFN, norm) over given key / value projections K, V (2-D views
        [B * nk, 256], free row strides) with every intermediate kept; returns (tape, output).
        `drop` (an `FfnDropout` carrying this layer's index, or None): the FFN's two training-mode
        dropouts; the tape then keeps the DROPPED, scaled hidden rows in s["h"]."""
        w, E = self.head.w, self._E
        M = B * nq
        ac, as_ = pre + "attentions.0.attn.", pre + "attentions.1.attn."
        Wc, bc = w[ac + "in_proj_weight"], w[ac + "in_proj_bias"]
        Ws, bs = w[as_ + "in_proj_weight"], w[as_ + "in_proj_bias"]
        s = dict(x_in=x, K=K, V=V, bits=bits, rowall=rowall, drop=drop)
        # cross-attention
        s["xp"] = E(M, 256)
        hip.add_periodic(x, qpos, s["xp"])
        s["Qc"] = E(M, 256)
        hip.linear(s["xp"], Wc[:256], bc[:256], s["Qc"])
        s["att_c"] = E(M, 256)
        hip.attention(s["Qc"], 256, K, K.stride(0), V, V.stride(0), bits, rowall, s["att_c"], 256,
                      scr, B, nq, nk, self.scale)
        s["y1"] = E(M, 256)
        hip.linear(s["att_c"], w[ac + "out_proj.weight"], w[ac + "out_proj.bias"], s["y1"], res=x)
        s["x1"] = E(M, 256)
        hip.layernorm(s["y1"], w[pre + "norms.0.weight"], w[pre + "norms.0.bias"], s["x1"])
        # self-attention
        s["x1p"] = E(M, 256)
        hip.add_periodic(s["x1"], qpos, s["x1p"])
        s["QKVs"] = E(M, 768)                               # columns [Q | K | V]
        hip.linear(s["x1p"], Ws[:512], bs[:512], s["QKVs"][:, :512])
        hip.linear(s["x1"], Ws[512:], bs[512:], s["QKVs"][:, 512:])
        s["att_s"] = E(M, 256)
        hip.attention(s["QKVs"], 768, s["QKVs"][:, 256:], 768, s["QKVs"][:, 512:], 768, None,
                      None, s["att_s"], 256, scr, B, nq, nq, self.scale)
        s["y2"] = E(M, 256)
        hip.linear(s["att_s"], w[as_ + "out_proj.weight"], w[as_ + "out_proj.bias"], s["y2"],
                   res=s["x1"])
        s["x2"] = E(M, 256)
        hip.layernorm(s["y2"], w[pre + "norms.1.weight"], w[pre + "norms.1.bias"], s["x2"])
        # FFN
        s["h"] = E(M, ffn)
        hip.linear(s["x2"], w[pre + "ffns.0.layers.0.0.weight"],
                   w[pre + "ffns.0.layers.0.0.bias"], s["h"], relu=True)
        s["y3"] = E(M, 256)
        if drop is None:
            hip.linear(s["h"], w[pre + "ffns.0.layers.1.weight"], w[pre + "ffns.0.layers.1.bias"],
                       s["y3"], res=s["x2"])
        else:
            drop.apply(s["h"], s["h"], 0)       # what layers.1 consumes and its d W contracts with
            hip.linear(s["h"], w[pre + "ffns.0.layers.1.weight"], w[pre + "ffns.0.layers.1.bias"],
                       s["y3"])
            drop.apply(s["y3"], s["y3"], 1, res=s["x2"])          # y3 = x2 + drop(layers.1 out)
        out = E(M, 256)
        hip.layernorm(s["y3"], w[pre + "norms.2.weight"], w[pre + "norms.2.bias"], out)
        return s, out

    def _layer_bwd(self, pre, s, dx, grads, B, nq, nk, scr, dqpos_rows, keysplit=False,
                   ks_scr=None):
        """Backward of `_layer_fwd`: accumulates the layer's parameter gradients and d (x +
        query_pos) (all three uses) into `dqpos_rows`; returns (d input, d K, d V).  `keysplit`:
        the masked cross-attention goes through `pn_mha_bwd_keysplit_masked_f32` (scratch `ks_scr`)
        under the layer's own bits / rowall instead of `pn_mha_bwd_f32` (scratch `scr`); the
        self-attention always takes the latter."""
        w, E = self.head.w, self._E
        M = B * nq
        ac, as_ = pre + "attentions.0.attn.", pre + "attentions.1.attn."
        Wc, Ws = w[ac + "in_proj_weight"], w[as_ + "in_proj_weight"]
        # norm2 <- FFN
        dy3 = self._ln_bwd(dx, s["y3"], pre + "norms.2.", grads)
        # dropout is linear: its backward is the same launch on the gradient (the forward's
        # counter, kept in the tape); the shortcut's share of dy3 stays un-dropped
        drop = s["drop"]
        dz = dy3
        if drop is not None:
            dz = E(M, 256)
            drop.apply(dy3, dz, 1)
        dh = self._lin_bwd(dz, s["h"], w[pre + "ffns.0.layers.1.weight"], grads,
                           pre + "ffns.0.layers.1.weight", pre + "ffns.0.layers.1.bias")
        if drop is not None:
            drop.apply(dh, dh, 0)
        hip.relu_bwd(dh, s["h"], dh)       # (saved h > 0 <=> kept and pre-activation > 0)
        dx2 = self._lin_bwd(dh, s["x2"], w[pre + "ffns.0.layers.0.0.weight"], grads,
                            pre + "ffns.0.layers.0.0.weight", pre + "ffns.0.layers.0.0.bias")
        self._acc(dx2, dy3)                                   # the FFN's identity shortcut
        # norm1 <- self-attention
        dy2 = self._ln_bwd(dx2, s["y2"], pre + "norms.1.", grads)
        datt = self._lin_bwd(dy2, s["att_s"], w[as_ + "out_proj.weight"], grads,
                             as_ + "out_proj.weight", as_ + "out_proj.bias")
        dQKV = E(M, 768)
        hip.mha_bwd(s["QKVs"], s["QKVs"][:, 256:], s["QKVs"][:, 512:], datt, dQKV,
                    dQKV[:, 256:], dQKV[:, 512:], scr, B, nq, nq, self.scale)
        dx1p = self._lin_bwd(dQKV[:, :512], s["x1p"], Ws[:512], grads, as_ + "in_proj_weight",
                             as_ + "in_proj_bias", row0=0)
        dx1 = self._lin_bwd(dQKV[:, 512:], s["x1"], Ws[512:], grads, as_ + "in_proj_weight",
                            as_ + "in_proj_bias", row0=512)
        self._acc(dx1, dx1p)
        self._acc(dqpos_rows, dx1p)
        self._acc(dx1, dy2)                                   # identity shortcut
        # norm0 <- cross-attention
        dy1 = self._ln_bwd(dx1, s["y1"], pre + "norms.0.", grads)
        datt = self._lin_bwd(dy1, s["att_c"], w[ac + "out_proj.weight"], grads,
                             ac + "out_proj.weight", ac + "out_proj.bias")
        dQc, dK, dV = E(M, 256), E(B * nk, 256), E(B * nk, 256)
        if keysplit:
            hip.mha_bwd_keysplit(s["Qc"], s["K"], s["V"], datt, dQc, dK, dV, ks_scr, B, nq, nk,
                                 self.scale, bits=s["bits"], rowall=s["rowall"])
        else:
            hip.mha_bwd(s["Qc"], s["K"], s["V"], datt, dQc, dK, dV, scr, B, nq, nk, self.scale,
                        bits=s["bits"], rowall=s["rowall"])
        dxp = self._lin_bwd(dQc, s["xp"], Wc[:256], grads, ac + "in_proj_weight",
                            ac + "in_proj_bias", row0=0)
        self._acc(dqpos_rows, dxp)
        self._acc(dxp, dy1)                                   # identity shortcut
        return dxp, dK, dV

    def _layer_fwd_self_first(self, pre, x, qpos, K, V, B, nq, nk, ffn, scr, drop=None):
        """`_layer_fwd` in the sibling head's operation order (baseline.py:363-386: self-attention,
        norm, cross-attention, norm, FFN, norm), unmasked.  mmcv numbers by position: attentions.0
        is the SELF-attention and norms.0 follows it, attentions.1 is the cross-attention.  The
        tape keeps the same keys as `_layer_fwd` (y1 / x1: behind the first attention, here the
        self-attention; y2 / x2: behind the second)."""
        w, E = self.head.w, self._E
        M = B * nq
        as_, ac = pre + "attentions.0.attn.", pre + "attentions.1.attn."
        Ws, bs = w[as_ + "in_proj_weight"], w[as_ + "in_proj_bias"]
        Wc, bc = w[ac + "in_proj_weight"], w[ac + "in_proj_bias"]
        s = dict(x_in=x, K=K, V=V, drop=drop)
        # self-attention
        s["xp"] = E(M, 256)
        hip.add_periodic(x, qpos, s["xp"])
        s["QKVs"] = E(M, 768)                               # columns [Q | K | V]
        hip.linear(s["xp"], Ws[:512], bs[:512], s["QKVs"][:, :512])
        hip.linear(x, Ws[512:], bs[512:], s["QKVs"][:, 512:])
        s["att_s"] = E(M, 256)
        hip.attention(s["QKVs"], 768, s["QKVs"][:, 256:], 768, s["QKVs"][:, 512:], 768, None,
                      None, s["att_s"], 256, scr, B, nq, nq, self.scale)
        s["y1"] = E(M, 256)
        hip.linear(s["att_s"], w[as_ + "out_proj.weight"], w[as_ + "out_proj.bias"], s["y1"], res=x)
        s["x1"] = E(M, 256)
        hip.layernorm(s["y1"], w[pre + "norms.0.weight"], w[pre + "norms.0.bias"], s["x1"])
        # cross-attention
        s["x1p"] = E(M, 256)
        hip.add_periodic(s["x1"], qpos, s["x1p"])
        s["Qc"] = E(M, 256)
        hip.linear(s["x1p"], Wc[:256], bc[:256], s["Qc"])
        s["att_c"] = E(M, 256)
        hip.attention(s["Qc"], 256, K, K.stride(0), V, V.stride(0), None, None, s["att_c"], 256,
                      scr, B, nq, nk, self.scale)
        s["y2"] = E(M, 256)
        hip.linear(s["att_c"], w[ac + "out_proj.weight"], w[ac + "out_proj.bias"], s["y2"],
                   res=s["x1"])
        s["x2"] = E(M, 256)
        hip.layernorm(s["y2"], w[pre + "norms.1.weight"], w[pre + "norms.1.bias"], s["x2"])
        # FFN
        s["h"] = E(M, ffn)
        hip.linear(s["x2"], w[pre + "ffns.0.layers.0.0.weight"],
                   w[pre + "ffns.0.layers.0.0.bias"], s["h"], relu=True)
        s["y3"] = E(M, 256)
        if drop is None:
            hip.linear(s["h"], w[pre + "ffns.0.layers.1.weight"], w[pre + "ffns.0.layers.1.bias"],
                       s["y3"], res=s["x2"])
        else:
            drop.apply(s["h"], s["h"], 0)
            hip.linear(s["h"], w[pre + "ffns.0.layers.1.weight"], w[pre + "ffns.0.layers.1.bias"],
                       s["y3"])
            drop.apply(s["y3"], s["y3"], 1, res=s["x2"])
        out = E(M, 256)
        hip.layernorm(s["y3"], w[pre + "norms.2.weight"], w[pre + "norms.2.bias"], out)
        return s, out

    def _layer_bwd_self_first(self, pre, s, dx, grads, B, nq, nk, scr, dqpos_rows, dK, dV,
                              keysplit=False, ks_scr=None):
        """Backward of `_layer_fwd_self_first`; d K / d V are written into the given 2-D views
        [B * nk, 256] (free row strides).  `keysplit`: the cross-attention goes through
        `pn_mha_bwd_keysplit_f32` (scratch `ks_scr`) instead of `pn_mha_bwd_f32` (scratch `scr`);
        the self-attention always takes the latter.  Returns d input."""
        w, E = self.head.w, self._E
        M = B * nq
        as_, ac = pre + "attentions.0.attn.", pre + "attentions.1.attn."
        Ws, Wc = w[as_ + "in_proj_weight"], w[ac + "in_proj_weight"]
        # norm2 <- FFN (as `_layer_bwd`)
        dy3 = self._ln_bwd(dx, s["y3"], pre + "norms.2.", grads)
        drop = s["drop"]
        dz = dy3
        if drop is not None:
            dz = E(M, 256)
            drop.apply(dy3, dz, 1)
        dh = self._lin_bwd(dz, s["h"], w[pre + "ffns.0.layers.1.weight"], grads,
                           pre + "ffns.0.layers.1.weight", pre + "ffns.0.layers.1.bias")
        if drop is not None:
            drop.apply(dh, dh, 0)
        hip.relu_bwd(dh, s["h"], dh)
        dx2 = self._lin_bwd(dh, s["x2"], w[pre + "ffns.0.layers.0.0.weight"], grads,
                            pre + "ffns.0.layers.0.0.weight", pre + "ffns.0.layers.0.0.bias")
        self._acc(dx2, dy3)                                   # the FFN's identity shortcut
        # norm1 <- cross-attention
        dy2 = self._ln_bwd(dx2, s["y2"], pre + "norms.1.", grads)
        datt = self._lin_bwd(dy2, s["att_c"], w[ac + "out_proj.weight"], grads,
                             ac + "out_proj.weight", ac + "out_proj.bias")
        dQc = E(M, 256)
        if keysplit:
            hip.mha_bwd_keysplit(s["Qc"], s["K"], s["V"], datt, dQc, dK, dV, ks_scr, B, nq, nk,
                                 self.scale)
        else:
            hip.mha_bwd(s["Qc"], s["K"], s["V"], datt, dQc, dK, dV, scr, B, nq, nk, self.scale)
        dx1p = self._lin_bwd(dQc, s["x1p"], Wc[:256], grads, ac + "in_proj_weight",
                             ac + "in_proj_bias", row0=0)
        self._acc(dqpos_rows, dx1p)
        self._acc(dx1p, dy2)                                  # identity shortcut: d x1
        # norm0 <- self-attention
        dy1 = self._ln_bwd(dx1p, s["y1"], pre + "norms.0.", grads)
        datt = self._lin_bwd(dy1, s["att_s"], w[as_ + "out_proj.weight"], grads,
                             as_ + "out_proj.weight", as_ + "out_proj.bias")
        dQKV = E(M, 768)
        hip.mha_bwd(s["QKVs"], s["QKVs"][:, 256:], s["QKVs"][:, 512:], datt, dQKV,
                    dQKV[:, 256:], dQKV[:, 512:], scr, B, nq, nq, self.scale)
        dxp = self._lin_bwd(dQKV[:, :512], s["xp"], Ws[:512], grads, as_ + "in_proj_weight",
                            as_ + "in_proj_bias", row0=0)
        dxin = self._lin_bwd(dQKV[:, 512:], s["x_in"], Ws[512:], grads, as_ + "in_proj_weight",
                             as_ + "in_proj_bias", row0=512)
        self._acc(dqpos_rows, dxp)
        self._acc(dxin, dxp)
        self._acc(dxin, dy1)                                  # identity shortcut
        return dxin

    def _relation_forward(self, pair, B, dropout=None):
        """The six Relation Fusion layers over `pair` [B * 2R, 256] with every intermediate kept."""
        head, w, E = self.head, self.head.w, self._E
        R, t = self.R, self.t
        M, Mk = B * R, B * 2 * R
        rpos, ppos = w["rel_query_embed.weight"], w["rel_query_embed2.weight"]
        t["pair"] = pair
        pairp = E(Mk, 256)                       # pair + key_pos (the keys' operand)
        hip.add_periodic(pair, ppos, pairp)
        t["pairp"] = pairp
        x = head._const(B)["r0"]                 # rel_query_feat repeated over the batch
        layers = []
        scr = E(max(hip.attn_scratch_floats(B, R, 2 * R), hip.attn_scratch_floats(B, R, R)))
        for i in range(self.L):
            pre = "relation_decoder.layers.%d." % i
            ac = pre + "attentions.0.attn."
            Wc, bc = w[ac + "in_proj_weight"], w[ac + "in_proj_bias"]
            KV = E(Mk, 512)                                     # columns [K | V]
            hip.linear(pairp, Wc[256:512], bc[256:512], KV[:, :256])
            hip.linear(pair, Wc[512:], bc[512:], KV[:, 256:])
            s, x = self._layer_fwd(pre, x, rpos, KV[:, :256], KV[:, 256:], B, R, 2 * R, self.ffn,
                                   scr, drop=self._drop_of(dropout, i))
            layers.append(s)
        t["layers"], t["r_out"] = layers, x
        C = w["rel_cls_embed.weight"].shape[0]
        rel = E(B, R, C)
        hip.linear(x, w["rel_cls_embed.weight"], w["rel_cls_embed.bias"], rel.view(M, C))
        t["rel"] = rel
        return rel

    @staticmethod
    def _drop_of(dropout, layer):
        """The descriptor of one layer, or None for no dropout (None, or rate 0: the plain layer's launches)."""
        if dropout is None or dropout.p == 0.0:
            return None
        return dropout._replace(layer=layer)

    # ------------------------------------------------------------------ backward
    @torch.no_grad()
    @hip.on_device
    def backward(self, g_rel=None, g_importance=None, g_sub=None, g_obj=None, cls_detached=True,
                 on_ready=None):
        """`cls_detached` (default: the reference's graph): pairnet_head.py:380-390 gathers the
        subject / object class logits from `cls_pred.clone().detach()`, so `loss_sub_cls` and
        `loss_obj_cls` reach no parameter -- `g_sub` / `g_obj` are accepted and, like autograd
        does there, contribute nothing.  With `cls_detached=False` they are propagated through
        the gathers, `cls_embed` and `post_norm` (the derivative of the un-detached expression).
        The gradients are views of `self.flat_grad` (valid until the next backward);
        `on_ready(end)`: called whenever flat_grad[:end] has become final (a reducer's hook)."""
        dq, grads = self._backward_tail(g_rel, g_importance, g_sub, g_obj, cls_detached, on_ready)
        if on_ready is not None:
            on_ready(self.flat_numel)
        return dq, grads

    def _backward_tail(self, g_rel, g_importance, g_sub, g_obj, cls_detached, on_ready):
        if self.t is None:
            raise RuntimeError("backward() needs a forward() first")
        t, B, Q, R = self.t, self.t["B"], self.Q, self.R
        grads = self._zero_grads()
        dq = self._zeros(B * Q, 256)
        prep = lambda g: g.to(self.dev, torch.float32).contiguous()
        ready = on_ready if on_ready is not None else (lambda end: None)
        if g_rel is not None:
            # ... and the gather of the pair features back onto the query rows (:342-351)
            dpair = self._relation_backward(prep(g_rel), grads, on_ready)
            hip.scatter_rows_add(dpair, t["pair_idx"], dq, B, Q, 2 * R, 256, accumulate=True)
        ready(self.group_end["rel_query"])
        if g_importance is not None:
            self._ppn_backward(prep(g_importance), grads, dq)
        ready(self.group_end["obj_query_update"])
        if not cls_detached and (g_sub is not None or g_obj is not None):
            self._cls_backward(g_sub, g_obj, grads, dq)
        return dq, grads

    @torch.no_grad()
    @hip.on_device
    def relation_forward(self, pair, dropout=None):
        """The Relation Fusion decoder alone: pair features [B * 2R, 256] (per image the R
        subject rows, then the R object rows) -> relation logits [B, R, C], taped.  `dropout`:
        an `FfnDropout` (the FFNs' training-mode dropout), default None."""
        B = pair.shape[0] // (2 * self.R)
        self.t = dict(B=B, q=None)
        return self._relation_forward(pair.contiguous(), B, dropout)

    @torch.no_grad()
    @hip.on_device
    def relation_backward(self, g_rel):
        """-> (d pair features [B * 2R, 256], {parameter name: gradient}) of the last
        `relation_forward` / `forward`."""
        grads = self._zero_grads()
        return self._relation_backward(g_rel.to(self.dev, torch.float32).contiguous(), grads), grads

    def _relation_backward(self, g_rel, grads, on_ready=None):
        w, E, t = self.head.w, self._E, self.t
        B, Q, R = t["B"], self.Q, self.R
        M, Mk = B * R, B * 2 * R
        C = g_rel.shape[-1]
        ready = on_ready if on_ready is not None else (lambda end: None)
        dx = self._lin_bwd(g_rel.view(M, C), t["r_out"], w["rel_cls_embed.weight"], grads,
                           "rel_cls_embed.weight", "rel_cls_embed.bias")
        ready(self.group_end["rel_cls_embed"])
        dpair, dpairp = self._zeros(Mk, 256), self._zeros(Mk, 256)   # d pair, d (pair + key_pos)
        drpos_rows = self._zeros(M, 256)                        # d (x + query_pos), all uses
        scr = E(max(hip.mha_bwd_scratch_floats(B, R, 2 * R), hip.mha_bwd_scratch_floats(B, R, R)))
        for i in reversed(range(self.L)):
            pre = "relation_decoder.layers.%d." % i
            ac = pre + "attentions.0.attn."
            Wc = w[ac + "in_proj_weight"]
            dx, dK, dV = self._layer_bwd(pre, t["layers"][i], dx, grads, B, R, 2 * R, scr,
                                         drpos_rows)
            dkp = self._lin_bwd(dK, t["pairp"], Wc[256:512], grads, ac + "in_proj_weight",
                                ac + "in_proj_bias", row0=256)
            self._acc(dpairp, dkp)
            dv = self._lin_bwd(dV, t["pair"], Wc[512:], grads, ac + "in_proj_weight",
                               ac + "in_proj_bias", row0=512)
            self._acc(dpair, dv)
            ready(self.group_end["relation_decoder.layers.%d" % i])
        # layer 0's input is rel_query_feat repeated over the batch
        hip.batch_sum(dx, grads["rel_query_feat.weight"], B)
        hip.batch_sum(drpos_rows, grads["rel_query_embed.weight"], B)
        hip.batch_sum(dpairp, grads["rel_query_embed2.weight"], B)
        self._acc(dpair, dpairp)
        return dpair

    def _mlp3_bwd(self, d_out, x, saved, prefix, grads):
        """Linear-ReLU-Linear-ReLU-Linear backward; saved = (h1, h2, out)."""
        w = self.head.w
        h1, h2, _ = saved
        d2 = self._lin_bwd(d_out, h2, w[prefix + ".4.weight"], grads, prefix + ".4.weight",
                           prefix + ".4.bias")
        hip.relu_bwd(d2, h2, d2)
        d1 = self._lin_bwd(d2, h1, w[prefix + ".2.weight"], grads, prefix + ".2.weight",
                           prefix + ".2.bias")
        hip.relu_bwd(d1, h1, d1)
        return self._lin_bwd(d1, x, w[prefix + ".0.weight"], grads, prefix + ".0.weight",
                             prefix + ".0.bias")

    def _ppn_backward(self, g_imp, grads, dq):
        w, E, t = self.head.w, self._E, self.t
        B, Q = t["B"], self.Q
        ml = "update_importance.conv_layers."
        c1, c2, raw = t["c1"], t["c2"], t["raw"]
        npix = B * Q * Q
        # ---- last layer (64 -> 1) ----
        part = E(B * Q, 49 * 64)
        hip.tapcorr1(c2, g_imp, part, B, Q, -1)
        dw3 = E(49 * 64)                                          # [tap][ci]
        hip.colsum(part, dw3)
        db3 = E(1)
        hip.colsum(g_imp.view(npix, 1), db3)
        dc2 = E(B, Q, Q, 64)
        hip.mlearner_last_bwd_data(g_imp, w[ml + "2.0.weight"], c2, dc2, B, Q)
        # ---- middle layer (64 -> 64) ----
        rows_per = 10
        chunks = B * ((Q + rows_per - 1) // rows_per)
        part2 = E(chunks, 64 * 49 * 64)
        hip.conv_wgrad(dc2, c1, part2, B, Q, Q, Q, Q, 64, 64, 7, 1, 3, rows_per)
        dw2 = E(64 * 49 * 64)                                     # [co][tap][ci]
        hip.colsum(part2, dw2)
        db2 = E(64)
        hip.colsum(dc2.view(npix, 64), db2)
        w2b = E(64 * 49 * 64)
        hip.conv_weight_bwd_layout(w[ml + "1.0.weight"], w2b, 64, 49, 64)
        dc1 = E(B, Q, Q, 64)
        hip.conv2d_ex(dc2, w2b.view(64, 49 * 64), None, None, dc1, B, Q, Q, 64, 64, 7, 7, 1, 3)
        hip.relu_bwd(dc1, c1, dc1)
        # ---- first layer (1 -> 64) ----
        hip.tapcorr1(dc1, raw, part, B, Q, +1)
        dw1t = E(49 * 64)                                         # [tap][co]
        hip.colsum(part, dw1t)
        db1 = E(64)
        hip.colsum(dc1.view(npix, 64), db1)
        w1b = E(49 * 64)
        hip.conv_weight_bwd_layout(w[ml + "0.0.weight"], w1b, 64, 49, 1)    # [1][49 flipped][64]
        draw = E(B, Q, Q)
        zero = self._zeros(1)
        hip.mlearner_last(dc1, w1b.view(49, 64), zero, draw, B, Q)
        # parameter gradients in the reference's layouts (cnn_factory.py: Conv2d weights [Co][Ci][7][7])
        # (copies that only re-order: [tap][ci] -> [1][ci][7][7], [co][tap][ci] -> [co][ci][7][7], ...)
        grads[ml + "2.0.weight"].copy_(dw3.view(49, 64).t().reshape(1, 64, 7, 7))
        grads[ml + "2.0.bias"].copy_(db3)
        grads[ml + "1.0.weight"].copy_(dw2.view(64, 7, 7, 64).permute(0, 3, 1, 2))
        grads[ml + "1.0.bias"].copy_(db2)
        grads[ml + "0.0.weight"].copy_(dw1t.view(49, 64).t().reshape(64, 1, 7, 7))
        grads[ml + "0.0.bias"].copy_(db1)
        # ---- cosine block + F.normalize ----
        s_e, o_e = t["sub"][2], t["obj"][2]
        s_hat, o_hat = E(B * Q, 256), E(B * Q, 256)
        hip.l2normalize(s_e, s_hat)
        hip.l2normalize(o_e, o_hat)
        ds, do = E(B * Q, 256), E(B * Q, 256)
        hip.cosine_bwd(draw, s_e, o_hat, ds, B, Q, False)
        hip.cosine_bwd(draw, o_e, s_hat, do, B, Q, True)
        self._acc(dq, self._mlp3_bwd(ds, t["q"], t["sub"], "sub_query_update", grads))
        self._acc(dq, self._mlp3_bwd(do, t["q"], t["obj"], "obj_query_update", grads))

    def _cls_backward(self, g_sub, g_obj, grads, dq):
        w, t = self.head.w, self.t
        B, Q, R = t["B"], self.Q, self.R
        nc = self.head.num_classes + 1
        # (scattered straight into the width `_lin_bwd` pads a ragged head to: no second copy)
        dcls = self._zeros(B * Q, (nc + 3) // 4 * 4)
        for g, pos in ((g_sub, t["sub_pos"]), (g_obj, t["obj_pos"])):
            if g is not None:
                g = g.to(self.dev, torch.float32).contiguous().view(B * R, nc)
                hip.scatter_rows_add(g, pos, dcls, B, Q, R, nc, accumulate=True)
        dqn = self._lin_bwd(dcls, t["qn"], w["cls_embed.weight"], grads, "cls_embed.weight",
                            "cls_embed.bias")
        self._acc(dq, self._ln_bwd(dqn, t["q"], "transformer_decoder.post_norm.", grads))


class HeadGrad(RelationTailGrad):
    """RelationTailGrad + the nine masked-attention decoder layers in front of it
    (pairnet_head.py:289-320; the reference's `transformer_decoder`, trained at lr_mult 0.1):
    everything of CrossHead2 that the reference's loss reaches behind the pixel decoder.

        tape = HeadGrad(head); head.forward(feats, metas); pl = head._last_plan
        out = tape.forward_from_plan(pl)               # re-runs the query chain with a tape
        dmem, grads = tape.backward(g_rel, g_importance)

    `forward_from_plan` needs a plan whose stage A has run (`head.forward`): the memory tokens
    `pl.X`, the K / V projections of the nine layers, the stencil rows of the mask feature.  The
    boolean attention masks (:244-256, `detach()`ed in the reference) are recomputed per layer by
    the product's own fused kernel and kept as packed bits.  `backward` returns the gradient with
    respect to the pixel decoder's memory tokens [B, sum_l N_l, 256] (what
    `PixelDecoderGrad.backward` takes) and the parameter gradients incl. `query_feat`,
    `query_embed`, `level_embed` and the cross-attentions' K / V projection rows."""

    @staticmethod
    def param_groups(head):
        groups = [g for g in RelationTailGrad.param_groups(head) if g[0] != "cls"]
        for i in reversed(range(head.num_dec_layers)):
            groups.append(("transformer_decoder.layers.%d" % i,
                           RelationTailGrad._layer_names("transformer_decoder.layers.%d." % i)))
        groups.append(("query", ["query_feat.weight", "query_embed.weight", "level_embed.weight"]))
        groups.append(RelationTailGrad.CLS_GROUP)
        return groups

    @torch.no_grad()
    @hip.on_device
    def forward_from_plan(self, pl, sub_pos=None, obj_pos=None, dropout=None):
        """`dropout` reaches the Relation Fusion decoder only: the nine masked layers' rate is 0.0
        in the reference and their outputs feed the masks and the pair selection."""
        head, w, E = self.head, self.head.w, self._E
        B, Q = pl.B, self.Q
        full = head.exact_mask_order == "full"
        qpos = w["query_embed.weight"]
        x = pl.q0
        if full:
            head._head_embed(pl.q0, pl, False, True)
        scr = E(max([hip.attn_scratch_floats(B, Q, n) for n in pl.N] +
                    [hip.attn_scratch_floats(B, Q, Q)]))
        layers = []
        for i in range(head.num_dec_layers):
            l = i % 3
            head._attn_mask(pl, l, None, me=pl.me0 if (i == 0 and not full) else None)
            nw = (pl.N[l] + 31) // 32
            bits, rowall = pl.bits[:B * Q * nw].clone(), pl.rowall.clone()
            s, x = self._layer_fwd("transformer_decoder.layers.%d." % i, x, qpos,
                                   pl.Kp[i].view(B * pl.N[l], 256), pl.Vp[i].view(B * pl.N[l], 256),
                                   B, Q, pl.N[l], head.dec_ffn, scr, bits, rowall)
            s["level"] = l
            layers.append(s)
            if i + 1 < head.num_dec_layers:      # post_norm + mask_embed -> the next layer's mask
                head._head_embed(x, pl, False, full)
        self.dt = dict(layers=layers, pl=pl, q_out=x)
        return self.forward(x, sub_pos, obj_pos, dropout)

    @torch.no_grad()
    @hip.on_device
    def backward(self, g_rel=None, g_importance=None, g_sub=None, g_obj=None, cls_detached=True,
                 on_ready=None):
        """-> (d memory tokens [B, SN, 256], {parameter name: gradient}); `self.dq_out` keeps the
        gradient w.r.t. the decoder's output queries."""
        dq, grads = self._backward_tail(g_rel, g_importance, g_sub, g_obj, cls_detached, on_ready)
        self.dq_out = dq
        head, w, E = self.head, self.head.w, self._E
        ready = on_ready if on_ready is not None else (lambda end: None)
        pl, layers = self.dt["pl"], self.dt["layers"]
        B, Q = pl.B, self.Q
        dmem = self._zeros(B, pl.SN, 256)
        dqpos_rows = self._zeros(B * Q, 256)
        scr = E(max([hip.mha_bwd_scratch_floats(B, Q, n) for n in pl.N] +
                    [hip.mha_bwd_scratch_floats(B, Q, Q)]))
        le, dle = w["level_embed.weight"], grads["level_embed.weight"]
        dx = dq.clone()
        for i in reversed(range(head.num_dec_layers)):
            pre = "transformer_decoder.layers.%d." % i
            ac = pre + "attentions.0.attn."
            Wc = w[ac + "in_proj_weight"]
            s = layers[i]
            l, N = s["level"], pl.N[s["level"]]
            dx, dK, dV = self._layer_bwd(pre, s, dx, grads, B, Q, N, scr, dqpos_rows)
            # K = (mem_l + level_embed_l + pe_l) Wk^T + bk, V = (mem_l + level_embed_l) Wv^T + bv
            # (pairnet_head.py:278-287, :302-312), image by image: a level's tokens of one image
            # are contiguous rows of pl.X
            for b in range(B):
                mem = pl.X[b, pl.start[l]:pl.start[l] + N]
                memk, memv = E(N, 256), E(N, 256)
                hip.add_periodic(mem, pl.dec_kpos[l], memk)
                hip.add_periodic(mem, le[l:l + 1], memv)
                dmk = self._lin_bwd(dK[b * N:(b + 1) * N], memk, Wc[256:512], grads,
                                    ac + "in_proj_weight", ac + "in_proj_bias", row0=256)
                dmv = self._lin_bwd(dV[b * N:(b + 1) * N], memv, Wc[512:], grads,
                                    ac + "in_proj_weight", ac + "in_proj_bias", row0=512)
                self._acc(dmk, dmv)
                dm = dmem[b, pl.start[l]:pl.start[l] + N]
                self._acc(dm, dmk)
                hip.colsum(dmk, dle[l], accumulate=True)      # level_embed_l feeds K and V
            ready(self.group_end["transformer_decoder.layers.%d" % i])
        hip.batch_sum(dx, grads["query_feat.weight"], B)
        hip.batch_sum(dqpos_rows, grads["query_embed.weight"], B)
        ready(self.group_end["query"])
        ready(self.flat_numel)
        return dmem, grads


class BBoxTailGrad(RelationTailGrad):
    """The relation tail of `CrossHeadBBox` (bbox_head.py), taped: what `losses.backward()` reaches
    in the reference's box head.  pairnet_bbox_head.py:261 detaches the trunk's queries
    (`query_feats = hs.clone().detach()`) and :322-330 the class logits, so the graph holds
    `sub_query_update` / `obj_query_update`, `update_importance`, the six `relation_decoder`
    layers, `rel_query_feat`, `rel_query_pos_embed`, `rel_key_pos_embed` and `rel_cls_embed` --
    `CrossHead2`'s tail under other parameter names.

        tape = BBoxTailGrad(head); out = tape.forward(pl.q, pl.cls, pl.sub_pos, pl.obj_pos)
        _, grads = tape.backward(g_rel=..., g_importance=...)

    Starts from the plan's kept, detached query rows `pl.q` [B * 100, 256] and takes the kept class
    logits `pl.cls` as given: no `post_norm` / `cls_embed`, no class group in the layout.  The
    layout carries the reference's names; `rel_value_pos_embed` (dead weight) and the trunk get no
    gradient and are not in it.  d q is dropped (`backward` returns None in its place)."""

    # CrossHead2's names of the two embeddings (what the inherited kernels' composition writes to,
    # and what `CrossHeadBBox._pack` aliases in the weight dict) -> the reference's
    ALIASES = OrderedDict((("rel_query_embed.weight", "rel_query_pos_embed.weight"),
                           ("rel_query_embed2.weight", "rel_key_pos_embed.weight")))

    @staticmethod
    def param_groups(head):
        alias = BBoxTailGrad.ALIASES
        return [(g, [alias.get(n, n) for n in names])
                for g, names in RelationTailGrad.param_groups(head) if g != "cls"]

    def _zero_grads(self):
        grads = dict(super()._zero_grads())
        for a, n in self.ALIASES.items():
            grads[a] = self.grads[n]
        return grads

    @torch.no_grad()
    @hip.on_device
    def forward(self, q, cls, sub_pos=None, obj_pos=None, dropout=None):
        """q [B * 100, 256], cls [B, 100, nc] (the kept queries and their class logits, both
        detached in the reference) -> dict(rel, importance, importance_raw, sub, obj, cls, sub_pos,
        obj_pos); the pair list is the top-k of `importance` unless `sub_pos` / `obj_pos` are given."""
        Q = self.Q
        if not (q.is_cuda and q.dtype == torch.float32 and q.dim() == 2 and q.shape[1] == 256
                and q.is_contiguous() and q.shape[0] % Q == 0):
            raise RuntimeError("q must be a contiguous [B * Q, 256] fp32 device tensor")
        B = q.shape[0] // Q
        if cls.dim() != 3 or tuple(cls.shape[:2]) != (B, Q) or not cls.is_contiguous():
            raise RuntimeError("cls must be a contiguous [B, Q, nc] fp32 device tensor")
        self.t = dict(B=B, q=q)
        # the Pair Proposal Network (pairnet_bbox_head.py:268-279), the pair features and the
        # relation decoder (:281-320): the parent's stages
        imp, raw, sub_pos, obj_pos = self._ppn_forward(q, B, sub_pos, obj_pos)
        return self._pairs_forward(q, cls, imp, raw, sub_pos, obj_pos, dropout)

    @torch.no_grad()
    @hip.on_device
    def backward(self, g_rel=None, g_importance=None, on_ready=None):
        """-> (None, {reference parameter name: gradient}).  The class logits are detached
        (pairnet_bbox_head.py:322-330): `loss_sub_cls` / `loss_obj_cls` reach no parameter, so
        their logit gradients are not taken.  The gradients are views of `self.flat_grad`."""
        self._backward_tail(g_rel, g_importance, None, None, True, on_ready)
        if on_ready is not None:
            on_ready(self.flat_numel)
        return None, self.grads
