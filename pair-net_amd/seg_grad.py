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

Not carried further here: dMF into the mask-feature convolution and the FPN, dmem into the pixel
decoder (`PixelDecoderGrad.backward` takes it), the relation branch, `reduce_mean` across ranks, an
optimizer step.
"""
import torch

from . import hip
from .grad import HeadGrad, RelationTailGrad

__all__ = ["SegmenterHeadGrad"]


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
