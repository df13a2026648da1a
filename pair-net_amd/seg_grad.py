"""Backward of the segmentation losses through the class / mask heads and the nine masked decoder
layers: from the logit gradients that `Mask2FormerLoss.loss(..., grads={})` /
`CrossHeadBaseline.seg_losses` / `full_losses` return to

  * the parameters of `cls_embed`, `mask_embed`, `post_norm` and the nine masked decoder layers
    (with `query_feat`, `query_embed`, `level_embed`),
  * the gradient with respect to the mask feature, dMF [B, H2 * W2, 256],
  * the gradient with respect to the pixel decoder's memory tokens, dmem [B, SN, 256] (what
    `PixelDecoderGrad.backward` takes).

The reference reaches these through `torch.autograd` behind `losses.backward()`: every decoder layer's
output goes through the SHARED heads (`forward_head`, pairnet_head.py:236-243 / baseline.py:254-296:
post_norm -> cls_embed, post_norm -> mask_embed -> einsum with the mask feature), and every layer's
class / mask logits carry loss terms (deep supervision).  Here the query chain is replayed into a
tape as `HeadGrad` does, the heads are taped once for all L layer outputs as one [L * B * Q, 256]
chain, and `backward` walks it: the two products of the mask logits are csrc/seg_grad.hip's kernels
(on the loss's COMPACT mask gradient: matched rows only), the rest is `RelationTailGrad`'s linear /
LayerNorm / decoder-layer backward with the per-layer gradient added in after each layer.

The boolean attention masks are `detach()`ed in the reference (:256): no gradient flows through
them, and the heads' evaluation on the initial queries feeds only a mask, so it gets none.

`SegPixelDecoderGrad` takes both tensors on: dMF through `mask_feature`, `output_convs.0`,
`lateral_convs.0` and the bilinear upsampling of the finest memory level (whose adjoint adds a
second share to dmem), then `PixelDecoderGrad`'s walk through the encoder and the input
convolutions on the sum.

Not carried further here: the backbone below the feature gradients (`BackboneGrad` takes them), the
relation branch, `reduce_mean` across ranks, an optimizer step.
"""
import torch

from . import hip
from .grad import HeadGrad, PixelDecoderGrad, RelationTailGrad

__all__ = ["SegmenterHeadGrad", "SegPixelDecoderGrad"]


class SegmenterHeadGrad(HeadGrad):
    """tape = SegmenterHeadGrad(head); head.forward(...) (return_all_layers=True for the sibling
    head); out = tape.forward_from_plan(head._last_plan); losses -> grads;
    dmem, dMF, g = tape.backward(grads, counts=n_b).

    Works on any head with the shared Mask2Former trunk (`CrossHead2`, `CrossHeadBaseline`).  The
    gradients are views of one flat buffer (`flat_grad`, segments padded to 64 floats, groups in
    completion order, `on_ready(end)`), as the other tapes keep them."""

    HEADS_GROUP = ("heads", ["mask_embed.4.weight", "mask_embed.4.bias", "mask_embed.2.weight",
                             "mask_embed.2.bias", "mask_embed.0.weight", "mask_embed.0.bias",
                             "cls_embed.weight", "cls_embed.bias",
                             "transformer_decoder.post_norm.weight",
                             "transformer_decoder.post_norm.bias"])

    def __init__(self, head, flat=None, base=0):
        super().__init__(head, flat, base)
        self.st = None
        self._tables = {}

    @staticmethod
    def param_groups(head):
        groups = [SegmenterHeadGrad.HEADS_GROUP]
        for i in reversed(range(head.num_dec_layers)):
            groups.append(("transformer_decoder.layers.%d" % i,
                           RelationTailGrad._layer_names("transformer_decoder.layers.%d." % i)))
        groups.append(("query", ["query_feat.weight", "query_embed.weight", "level_embed.weight"]))
        return groups

    # ------------------------------------------------------------------ forward with a tape
    def forward(self, q_all, with_mask=False):
        """The shared heads on all L layer outputs at once: q_all [L * B * Q, 256] (layer-major,
        each layer's queries BEFORE post_norm) -> dict(cls [L, B, Q, C + 1], me [L * B * Q, 256]
        and, with `with_mask`, mask [L, B, Q, H2, W2])."""
        head, w, E = self.head, self.head.w, self._E
        pl = self.dt["pl"]
        B, Q, L = pl.B, self.Q, head.num_dec_layers
        N = L * B * Q
        nc = head.num_classes + 1
        qn, m1, m2, me = E(N, 256), E(N, 256), E(N, 256), E(N, 256)
        hip.layernorm(q_all, w["transformer_decoder.post_norm.weight"],
                      w["transformer_decoder.post_norm.bias"], qn)
        cls = E(L, B, Q, nc)
        hip.linear(qn, w["cls_embed.weight"], w["cls_embed.bias"], cls.view(N, nc))
        hip.linear(qn, w["mask_embed.0.weight"], w["mask_embed.0.bias"], m1, relu=True)
        hip.linear(m1, w["mask_embed.2.weight"], w["mask_embed.2.bias"], m2, relu=True)
        hip.linear(m2, w["mask_embed.4.weight"], w["mask_embed.4.bias"], me)
        self.st = dict(q=q_all, qn=qn, mlp=(m1, m2, me), B=B, L=L)
        out = dict(cls=cls, me=me)
        if with_mask:
            H2, W2 = pl.hw2
            mask = E(L, B, Q, H2, W2)
            for l in range(L):
                head._mask_logits(me[l * B * Q:(l + 1) * B * Q], pl, mask[l].view(B, Q, pl.HW2))
            out["mask"] = mask
        return out

    @torch.no_grad()
    @hip.on_device
    def forward_from_plan(self, pl, with_mask=False):
        """Replays the nine masked layers of a plan whose stage A has run (`head.forward`) into
        the tape -- the same mask bits and `exact_mask_order` handling as
        `HeadGrad.forward_from_plan` -- then tapes the heads of all layer outputs."""
        head, w, E = self.head, self.head.w, self._E
        B, Q, L = pl.B, self.Q, head.num_dec_layers
        full = head.exact_mask_order == "full"
        qpos = w["query_embed.weight"]
        x = pl.q0
        # (the plan's own logit buffer may be an output the caller still holds: "full" gets its own)
        mp = E(B, Q, pl.HW2) if full else None
        if full:
            head._head_embed(pl.q0, pl, False, True, mp_out=mp)
        scr = E(max([hip.attn_scratch_floats(B, Q, n) for n in pl.N] +
                    [hip.attn_scratch_floats(B, Q, Q)]))
        q_all = E(L * B * Q, 256)
        layers = []
        for i in range(L):
            l = i % 3
            head._attn_mask(pl, l, mp, me=pl.me0 if (i == 0 and not full) else None)
            nw = (pl.N[l] + 31) // 32
            bits, rowall = pl.bits[:B * Q * nw].clone(), pl.rowall.clone()
            s, x = self._layer_fwd("transformer_decoder.layers.%d." % i, x, qpos,
                                   pl.Kp[i].view(B * pl.N[l], 256), pl.Vp[i].view(B * pl.N[l], 256),
                                   B, Q, pl.N[l], head.dec_ffn, scr, bits, rowall)
            s["level"] = l
            layers.append(s)
            q_all[i * B * Q:(i + 1) * B * Q].copy_(x)
            if i + 1 < L:                        # post_norm + mask_embed -> the next layer's mask
                head._head_embed(x, pl, False, full, mp_out=mp)
        self.dt = dict(layers=layers, pl=pl, q_out=x)
        return self.forward(q_all, with_mask)

    # ------------------------------------------------------------------ backward
    def _table(self, L, counts):
        key = (L, tuple(counts))
        if key not in self._tables:
            host, T = hip.mask_grad_table(L, counts)
            if len(self._tables) >= 64:
                self._tables.clear()
            self._tables[key] = (host.pin_memory().to(self.dev, non_blocking=True), T)
        return self._tables[key]

    def _check_grads(self, grads, counts):
        st, pl = self.st, self.dt["pl"]
        B, L, Q = st["B"], st["L"], self.Q
        nc = self.head.num_classes + 1
        for k in ("cls", "mask", "mask_rows"):
            if k not in grads:
                raise ValueError("grads lacks %r (Mask2FormerLoss.loss(..., grads={}))" % k)
        g_cls, g_mask, rows = grads["cls"], grads["mask"], grads["mask_rows"]
        for t, dt in ((g_cls, torch.float32), (g_mask, torch.float32), (rows, torch.int64)):
            if not (torch.is_tensor(t) and t.is_cuda and t.device == self.dev and t.dtype == dt):
                raise ValueError("grads: fp32 / int64 tensors on %s" % self.dev)
        if tuple(g_cls.shape) != (L, B, Q, nc):
            raise ValueError("grads['cls'] %s does not match the tape's [%d, %d, %d, %d]"
                             % (tuple(g_cls.shape), L, B, Q, nc))
        M = int(rows.shape[0])
        if rows.dim() != 1 or g_mask.dim() != 3 or g_mask.shape[0] != M or \
                (M and tuple(g_mask.shape[1:]) != tuple(pl.hw2)):
            raise ValueError("grads['mask'] %s / ['mask_rows'] %s do not match the tape's [M, %d, %d]"
                             % (tuple(g_mask.shape), tuple(rows.shape), pl.hw2[0], pl.hw2[1]))
        if counts is None:
            if B != 1 or M % L:
                raise ValueError("counts: the matched rows per image (min(Q, G_b)), needed for B > 1")
            counts = [M // L]
        counts = [int(c) for c in counts]
        if len(counts) != B or min(counts) < 0 or max(counts) > Q or L * sum(counts) != M:
            raise ValueError("counts %s do not match %d images, %d queries and %d = L * sum rows"
                             % (counts, B, Q, M))
        return g_cls.contiguous(), g_mask.contiguous(), rows.contiguous(), counts

    @torch.no_grad()
    @hip.on_device
    def backward(self, grads, on_ready=None, counts=None):
        """`grads`: "cls" [L, B, Q, C + 1], "mask" [M, H2, W2] and "mask_rows" [M] as the
        segmentation loss fills them; `counts`: the matched rows per image n_b = min(Q, G_b) (the
        loss object's `last["counts"]`; optional for one image).  Nothing is read back from the
        device.  -> (dmem [B, SN, 256], dMF [B, H2 * W2, 256], {reference parameter name: gradient});
        `self.dq_all` [L, B * Q, 256] keeps the gradient that enters each layer's output from its
        own heads.  The gradients are views of `self.flat_grad`; `on_ready(end)` as `HeadGrad`."""
        if self.st is None:
            raise RuntimeError("backward() needs a forward_from_plan() first")
        g_cls, g_mask, rows, counts = self._check_grads(grads, counts)
        head, w, E, st = self.head, self.head.w, self._E, self.st
        pl, layers = self.dt["pl"], self.dt["layers"]
        B, Q, L = st["B"], self.Q, st["L"]
        N, M, P = L * B * Q, int(rows.shape[0]), pl.HW2
        nc = head.num_classes + 1
        ready = on_ready if on_ready is not None else (lambda end: None)
        zeros = lambda *s_: torch.zeros(*s_, device=self.dev, dtype=torch.float32)
        grads_out = self._zero_grads()
        me = st["mlp"][2]
        # ---- the mask logits' two products on the compact rows ----
        table, T = self._table(L, counts)
        G = g_mask.view(M, P)
        MF = pl.MF.view(B, P, 256)
        dMF = E(B, P, 256)
        hip.mask_feature_grad(G, me, rows, table, T, dMF)
        if M:
            dme = E(M, 256)
            hip.mask_embed_grad(G, MF, rows, table, T, dme,
                                E(hip.mask_embed_grad_scratch_floats(T, P)))
            # onto the L * B * Q rows (a matched row appears once; failed rows, -1, match none)
            dme_all = E(N, 256)
            hip.scatter_rows_add(dme, rows, dme_all, 1, N, M, 256)
        else:
            dme_all = zeros(N, 256)
        # ---- mask_embed, cls_embed, post_norm on all rows ----
        dqn = self._mlp3_bwd(dme_all, st["qn"], st["mlp"], "mask_embed", grads_out)
        ncp = (nc + 3) // 4 * 4           # the GEMMs contract over multiples of 4: zero columns
        dcls = zeros(N, ncp)
        dcls[:, :nc].copy_(g_cls.view(N, nc))
        Wp = zeros(ncp, 256)
        Wp[:nc].copy_(w["cls_embed.weight"])
        gp = {"W": zeros(ncp, 256), "b": zeros(ncp)}
        self._acc(dqn, self._lin_bwd(dcls, st["qn"], Wp, gp, "W", "b"))
        self._acc(grads_out["cls_embed.weight"], gp["W"][:nc])
        self._acc(grads_out["cls_embed.bias"], gp["b"][:nc])
        dq_all = self._ln_bwd(dqn, st["q"], "transformer_decoder.post_norm.", grads_out)
        self.dq_all = dq_all.view(L, B * Q, 256)
        ready(self.group_end["heads"])
        # ---- the nine layers, last to first, each layer's own head gradient added in ----
        dmem = zeros(B, pl.SN, 256)
        dqpos_rows = zeros(B * Q, 256)
        scr = E(max([hip.mha_bwd_scratch_floats(B, Q, n) for n in pl.N] +
                    [hip.mha_bwd_scratch_floats(B, Q, Q)]))
        le, dle = w["level_embed.weight"], grads_out["level_embed.weight"]
        dx = self.dq_all[L - 1].clone()
        for i in reversed(range(L)):
            pre = "transformer_decoder.layers.%d." % i
            ac = pre + "attentions.0.attn."
            Wc = w[ac + "in_proj_weight"]
            s = layers[i]
            l, Nk = s["level"], pl.N[s["level"]]
            dx, dK, dV = self._layer_bwd(pre, s, dx, grads_out, B, Q, Nk, scr, dqpos_rows)
            if i > 0:                            # deep supervision: layer i - 1's output has heads
                self._acc(dx, self.dq_all[i - 1])
            # K = (mem_l + level_embed_l + pe_l) Wk^T + bk, V = (mem_l + level_embed_l) Wv^T + bv
            # (pairnet_head.py:278-287, :302-312), image by image, as HeadGrad.backward
            for b in range(B):
                mem = pl.X[b, pl.start[l]:pl.start[l] + Nk]
                memk, memv = E(Nk, 256), E(Nk, 256)
                hip.add_periodic(mem, pl.dec_kpos[l], memk)
                hip.add_periodic(mem, le[l:l + 1], memv)
                dmk = self._lin_bwd(dK[b * Nk:(b + 1) * Nk], memk, Wc[256:512], grads_out,
                                    ac + "in_proj_weight", ac + "in_proj_bias", row0=256)
                dmv = self._lin_bwd(dV[b * Nk:(b + 1) * Nk], memv, Wc[512:], grads_out,
                                    ac + "in_proj_weight", ac + "in_proj_bias", row0=512)
                self._acc(dmk, dmv)
                dm = dmem[b, pl.start[l]:pl.start[l] + Nk]
                self._acc(dm, dmk)
                hip.colsum(dmk, dle[l], accumulate=True)      # level_embed_l feeds K and V
            ready(self.group_end["transformer_decoder.layers.%d" % i])
        hip.batch_sum(dx, grads_out["query_feat.weight"], B)
        hip.batch_sum(dqpos_rows, grads_out["query_embed.weight"], B)
        ready(self.group_end["query"])
        ready(self.flat_numel)
        return dmem, dMF, grads_out


class SegPixelDecoderGrad(PixelDecoderGrad):
    """`PixelDecoderGrad` plus the mask-feature branch the segmentation losses reach
    (MSDeformAttnPixelDecoder.forward behind pairnet_head.py:262: `lateral_convs.0` on C2, + the
    bilinear upsampling of the finest memory level, `output_convs.0`, `mask_feature`):

        tape = SegPixelDecoderGrad(head)
        mem, MF = tape.forward(feats)                      # MF [B, H2 * W2, 256]
        dfeats, grads = tape.backward(dmem, dMF, need_dc2=False)

    `dmem`, `dMF`: what `SegmenterHeadGrad.backward` returns.  `dfeats[0..2]` are the parent's (C5,
    C4, C3), `dfeats[3]` is d C2 [B, C, H2, W2] or None without `need_dc2` (the R50 config freezes
    layer1).  The upsampling's adjoint (`pn_bilinear_nhwc_bwd_f32`) adds the branch's share into the
    level-2 rows of a copy of `dmem`, and the parent's walk runs on that sum.  The 3x3 convolution
    is taped as the direct implicit GEMM (as `BackboneGrad` does), its data gradient is the forward
    convolution on the tap-reversed weight (`dgrad_algo`: Winograd F(4x4, 3x3), the faster form at
    200 x 334, or the direct kernel), its weight gradient `pn_conv_wgrad_f32`; the two GroupNorms go
    back through `pn_groupnorm_act_nhwc_bwd_f32` (the ReLU's gate from the saved output).  The three
    new parameter groups come first in the flat buffer, in completion order.

    The branch's own results -- its eight gradients, d C2 and `self.dmem_sum`, the sum handed to
    the parent -- are bitwise reproducible.  The parent's walk is not, from the first
    `pn_msda_bwd_f32` on: that kernel adds grad_value with float atomics, like mmcv's
    (csrc/msda.hip), so everything behind layer 5's `value_proj` varies in its last bits from
    call to call, as `PixelDecoderGrad.backward`'s results always have."""

    BRANCH_GROUPS = [
        ("mask_feature", [PixelDecoderGrad.PD + "mask_feature." + n for n in ("weight", "bias")]),
        ("output_convs.0", [PixelDecoderGrad.PD + "output_convs.0." + n
                            for n in ("conv.weight", "gn.weight", "gn.bias")]),
        ("lateral_convs.0", [PixelDecoderGrad.PD + "lateral_convs.0." + n
                             for n in ("conv.weight", "gn.weight", "gn.bias")])]

    def __init__(self, head, flat=None, base=0):
        super().__init__(head, flat, base)
        self._zeroed = False
        self.dgrad_algo = "winograd4"   # the 3x3's data gradient: "winograd4" or "direct"

    @staticmethod
    def param_groups(head):
        return list(SegPixelDecoderGrad.BRANCH_GROUPS) + PixelDecoderGrad.param_groups(head)

    def _zero_grads(self):
        if not self._zeroed:            # (the parent's walk runs inside backward(): zeroed once)
            self.flat_grad.zero_()
        return self.grads

    # ------------------------------------------------------------------ forward with a tape
    @torch.no_grad()
    @hip.on_device
    def forward(self, feats):
        mem = PixelDecoderGrad.forward(self, feats)
        head, w, E, pd, t = self.head, self.head.w, self._E, self.PD, self.t
        B, SN, start = t["B"], t["SN"], t["start"]
        f = feats[0]
        cin, (H2, W2) = f.shape[1], f.shape[-2:]
        HW2, G = H2 * W2, head.gn_groups
        h2, w2 = t["shapes"][2]
        part = torch.empty(B * hip.groupnorm_nblk(HW2) * G * 2, device=self.dev,
                           dtype=torch.float64)
        rows = [self._rows(f[b]) for b in range(B)]
        lat = E(B, HW2, 256)
        for b in range(B):
            hip.linear(rows[b], w[pd + "lateral_convs.0.conv.weight"], None, lat[b])
        T = E(B, H2, W2, 256)
        hip.groupnorm_nhwc(lat, w[pd + "lateral_convs.0.gn.weight"],
                           w[pd + "lateral_convs.0.gn.bias"], T, part, B, HW2, G, False,
                           HW2 * 256, HW2 * 256)
        hip.bilinear_nhwc(mem[:, start[2]:], T, B, h2, w2, H2, W2, 256, True, SN * 256, HW2 * 256)
        c3 = E(B, H2, W2, 256)
        hip.conv2d_ex(T, w[pd + "output_convs.0.conv.weight"], None, None, c3, B, H2, W2, 256, 256,
                      3, 3, 1, 1)
        Y = E(B, H2, W2, 256)
        hip.groupnorm_nhwc(c3, w[pd + "output_convs.0.gn.weight"], w[pd + "output_convs.0.gn.bias"],
                           Y, part, B, HW2, G, True, HW2 * 256, HW2 * 256)
        MF = E(B, HW2, 256)
        hip.linear(Y.view(-1, 256), w[pd + "mask_feature.weight"], w[pd + "mask_feature.bias"],
                   MF.view(-1, 256))
        t["fpn"] = dict(rows=rows, lat=lat, T=T, c3=c3, Y=Y, hw2=(H2, W2), cin=cin)
        return mem, MF

    # ------------------------------------------------------------------ backward
    def _gn_bwd(self, x, dy, y, prefix, grads, B, HW, scratch, stats):
        """GroupNorm (+ReLU when `y`, its saved output, is given) backward -> dx [B * HW, 256];
        d weight / d bias accumulated."""
        dx = self._E(B * HW, 256)
        hip.groupnorm_act_nhwc_bwd(x, dy, y, self.head.w[prefix + "weight"], dx,
                                   grads[prefix + "weight"], grads[prefix + "bias"], stats, scratch,
                                   B, HW, self.head.gn_groups, y is not None, True, HW * 256,
                                   HW * 256)
        return dx

    def _check_upstream(self, dmem, dMF):
        t = self.t
        B, SN = t["B"], t["SN"]
        H2, W2 = t["fpn"]["hw2"]
        if self.dgrad_algo not in ("winograd4", "direct"):
            raise ValueError("dgrad_algo %r: 'winograd4' or 'direct'" % (self.dgrad_algo,))
        for name, g, shape in (("dmem", dmem, (B, SN, 256)), ("dMF", dMF, (B, H2 * W2, 256))):
            if not (torch.is_tensor(g) and g.is_cuda and g.device == self.dev and
                    g.dtype == torch.float32):
                raise ValueError("%s: an fp32 tensor on %s" % (name, self.dev))
            if tuple(g.shape) != shape:
                raise ValueError("%s %s does not match the tape's %s" % (name, tuple(g.shape), shape))
        return dmem.contiguous(), dMF.contiguous()

    @torch.no_grad()
    @hip.on_device
    def backward(self, dmem, dMF, need_dc2=False, on_ready=None):
        if self.t is None or "fpn" not in self.t:
            raise RuntimeError("backward() needs a forward() first")
        dmem, dMF = self._check_upstream(dmem, dMF)
        head, w, E, pd, t = self.head, self.head.w, self._E, self.PD, self.t
        B, SN, start, s = t["B"], t["SN"], t["start"], t["fpn"]
        (H2, W2), cin, G = s["hw2"], s["cin"], head.gn_groups
        HW2 = H2 * W2
        h2, w2 = t["shapes"][2]
        ready = on_ready if on_ready is not None else (lambda end: None)
        grads = self._zero_grads()
        scratch = hip.groupnorm_act_bwd_scratch(B, HW2, G, self.dev)
        stats = E(B * G * 4)
        # ---- mask_feature (a linear layer over pixels) ----
        dY = self._lin_bwd(dMF.view(-1, 256), s["Y"].view(-1, 256), w[pd + "mask_feature.weight"],
                           grads, pd + "mask_feature.weight", pd + "mask_feature.bias")
        ready(self.group_end["mask_feature"])
        # ---- output_convs.0: GroupNorm + ReLU, then the 3x3 convolution ----
        dc3 = self._gn_bwd(s["c3"], dY, s["Y"], pd + "output_convs.0.gn.", grads, B, HW2, scratch,
                           stats)
        del dY
        rows_per = max(1, min(H2, 8))
        chunks = B * ((H2 + rows_per - 1) // rows_per)
        part = E(chunks, 256 * 9 * 256)
        hip.conv_wgrad(dc3, s["T"], part, B, H2, W2, H2, W2, 256, 256, 3, 1, 1, rows_per)
        dwp = E(256 * 9 * 256)                                # [co][tap][ci]: the packed layout
        hip.colsum(part, dwp)
        del part
        grads[pd + "output_convs.0.conv.weight"].copy_(
            dwp.view(256, 3, 3, 256).permute(0, 3, 1, 2))     # -> [co][ci][3][3]
        ready(self.group_end["output_convs.0"])
        wb = E(256 * 9 * 256)
        hip.conv_weight_bwd_layout(w[pd + "output_convs.0.conv.weight"], wb, 256, 9, 256)
        dT = E(B, H2, W2, 256)
        if self.dgrad_algo == "winograd4":
            # F(4x4, 3x3) on the reversed weight: 0.29 against 0.72 ms at 200 x 334 (labnotes R20.4)
            U = hip.winograd43_weights(wb.view(256, 3, 3, 256).permute(0, 3, 1, 2).contiguous())
            tiles = B * ((H2 + 3) // 4) * ((W2 + 3) // 4)
            hip.conv3x3_winograd43(dc3, U, None, dT, E(36 * tiles * 256), E(36 * tiles * 256), B, H2,
                                   W2, 256, 256, False)
        elif self.dgrad_algo == "direct":
            hip.conv2d_ex(dc3, wb.view(256, 9 * 256), None, None, dT, B, H2, W2, 256, 256, 3, 3, 1, 1)
        else:
            raise ValueError("dgrad_algo %r: 'winograd4' or 'direct'" % (self.dgrad_algo,))
        del dc3
        # ---- dT splits: lateral_convs.0 (GroupNorm, 1x1 convolution on C2) ... ----
        dlat = self._gn_bwd(s["lat"], dT, None, pd + "lateral_convs.0.gn.", grads, B, HW2, scratch,
                            stats)
        dc2 = E(B, cin, H2, W2) if need_dc2 else None
        for b in range(B):
            drows = self._lin_bwd(dlat[b * HW2:(b + 1) * HW2], s["rows"][b],
                                  w[pd + "lateral_convs.0.conv.weight"], grads,
                                  pd + "lateral_convs.0.conv.weight", None, need_dx=need_dc2)
            if need_dc2:
                hip.transpose(drows, dc2[b].view(cin, HW2))
        ready(self.group_end["lateral_convs.0"])
        # ---- ... and the upsampling's adjoint into the finest level's rows of the memory ----
        dsum = dmem.clone()
        hip.bilinear_nhwc_bwd(dT, dsum[:, start[2]:], B, h2, w2, H2, W2, 256, True, HW2 * 256,
                              SN * 256)
        del dT
        self.dmem_sum = dsum                    # what enters the parent's walk (dmem + the branch's share)
        self._zeroed = True
        try:
            dfeats, grads = PixelDecoderGrad.backward(self, dsum, on_ready)
        finally:
            self._zeroed = False
        return dfeats + [dc2], grads
