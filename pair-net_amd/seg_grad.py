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

`BaselineHeadGrad` adds the sibling head's relation branch to the first tape: the "rel",
"subject_scores" and "object_scores" gradients of `full_losses` through `rel_cls_embed`, the cosine
scores, the two update MLPs and the six relation decoder layers (whose cross-attention backward over
a memory level is csrc/attn_grad.hip's key-split kernel), their shares added into the final queries'
gradient, dmem and `level_embed`.

`PSGTr2HeadGrad` is the same trunk under `PSGTrHead2`'s heads: no deep supervision, one head chain
over the last layer's output and the initial queries (`obj_mask_embed` is used on both), the three
ragged class heads' backward in csrc/tri_grad.hip's two launches.

Not carried further here: the backbone below the feature gradients (`BackboneGrad` takes them) and
the optimizer step (`BaselineTrainer`, baseline_train.py, and `PSGTr2Trainer`, psgtr2_train.py, run
both), `reduce_mean` across ranks.
"""
import torch

from . import hip
from .grad import HeadGrad, RelationTailGrad
from .pixel_grad import PixelDecoderGrad

__all__ = ["SegmenterHeadGrad", "BaselineHeadGrad", "PSGTr2HeadGrad", "SegPixelDecoderGrad"]


class SegmenterHeadGrad(HeadGrad):
    """tape = SegmenterHeadGrad(head); head.forward(...) (return_all_layers=True for the sibling
    head); out = tape.forward_from_plan(head._last_plan); losses -> grads;
    dmem, dMF, g = tape.backward(grads, counts=n_b).

    Works on any head with the shared Mask2Former trunk (`CrossHead2`, `CrossHeadBaseline`).  The
    gradients are views of one flat buffer (`flat_grad`, segments padded to 64 floats, groups in
    completion order, `on_ready(end)`), as the other tapes keep them.

    `masked_keysplit_min_keys` (default None): the nine masked cross-attentions' backward.  None is
    `pn_mha_bwd_f32` for every layer; an integer sends the layers whose memory level has at least
    that many keys through `pn_mha_bwd_keysplit_masked_f32` (csrc/attn_grad.hip) under the layer's
    own bits / rowall (faster from 4 200 keys on, slower at 1 050: labnotes R24.4)."""

    HEADS_GROUP = ("heads", ["mask_embed.4.weight", "mask_embed.4.bias", "mask_embed.2.weight",
                             "mask_embed.2.bias", "mask_embed.0.weight", "mask_embed.0.bias",
                             "cls_embed.weight", "cls_embed.bias",
                             "transformer_decoder.post_norm.weight",
                             "transformer_decoder.post_norm.bias"])

    def __init__(self, head, flat=None, base=0):
        super().__init__(head, flat, base)
        self.st = None
        self._tables = {}
        # the nine masked cross-attentions' backward: None (default) is `pn_mha_bwd_f32` everywhere,
        # today's launches and bits; an integer sends the layers whose memory level has at least
        # that many keys through `pn_mha_bwd_keysplit_masked_f32` (0: all nine)
        self.masked_keysplit_min_keys = None

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

    def _replay_layers(self, pl, keep=None):
        """The nine masked layers of a plan whose stage A has run, into the tape (`self.dt`): the
        same mask bits and `exact_mask_order` handling as `HeadGrad.forward_from_plan`.
        `keep(i, x)` sees every layer's output (before post_norm)."""
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
            if keep is not None:
                keep(i, x)
            if i + 1 < L:                        # post_norm + mask_embed -> the next layer's mask
                head._head_embed(x, pl, False, full, mp_out=mp)
        self.dt = dict(layers=layers, pl=pl, q_out=x)

    @torch.no_grad()
    @hip.on_device
    def forward_from_plan(self, pl, with_mask=False):
        """Replays the nine masked layers of a plan whose stage A has run (`head.forward`) into
        the tape (`_replay_layers`), then tapes the heads of all layer outputs."""
        B, Q, L = pl.B, self.Q, self.head.num_dec_layers
        q_all = self._E(L * B * Q, 256)
        self._replay_layers(pl, lambda i, x: q_all[i * B * Q:(i + 1) * B * Q].copy_(x))
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

    def _layers_bwd(self, dx, dqpos_rows, dmem, grads_out, ready, deep=None):
        """The walk through the nine masked layers, last to first: `dx` [B * Q, 256] enters the last
        layer's output; `deep` [L, B * Q, 256] (deep supervision) is the gradient each earlier
        layer's output receives from its own heads, added in after the layer above it, None for a
        head without it.  Adds into `dmem`, `dqpos_rows`, `level_embed` and the layers' gradients;
        -> the gradient into the initial queries."""
        head, w, E = self.head, self.head.w, self._E
        pl, layers = self.dt["pl"], self.dt["layers"]
        B, Q, L = pl.B, self.Q, head.num_dec_layers
        mk = self.masked_keysplit_min_keys
        ks_levels = [n for n in pl.N if mk is not None and n >= mk]
        scr = E(max([hip.mha_bwd_scratch_floats(B, Q, n) for n in pl.N if n not in ks_levels] +
                    [hip.mha_bwd_scratch_floats(B, Q, Q)]))
        ks_scr = E(max(hip.mha_bwd_keysplit_scratch_floats(B, Q, n) for n in ks_levels)) \
            if ks_levels else None                       # (allocated only when a layer uses it)
        le, dle = w["level_embed.weight"], grads_out["level_embed.weight"]
        for i in reversed(range(L)):
            pre = "transformer_decoder.layers.%d." % i
            ac = pre + "attentions.0.attn."
            Wc = w[ac + "in_proj_weight"]
            s = layers[i]
            l, Nk = s["level"], pl.N[s["level"]]
            if mk is not None and Nk >= mk:
                dx, dK, dV = self._layer_bwd(pre, s, dx, grads_out, B, Q, Nk, scr, dqpos_rows,
                                             True, ks_scr)
            else:
                dx, dK, dV = self._layer_bwd(pre, s, dx, grads_out, B, Q, Nk, scr, dqpos_rows)
            if i > 0 and deep is not None:       # deep supervision: layer i - 1's output has heads
                self._acc(dx, deep[i - 1])
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
        return dx

    @torch.no_grad()
    @hip.on_device
    def backward(self, grads, on_ready=None, counts=None, seed_dq=None, seed_dmem=None):
        """`grads`: "cls" [L, B, Q, C + 1], "mask" [M, H2, W2] and "mask_rows" [M] as the
        segmentation loss fills them; `counts`: the matched rows per image n_b = min(Q, G_b) (the
        loss object's `last["counts"]`; optional for one image).  Nothing is read back from the
        device.  -> (dmem [B, SN, 256], dMF [B, H2 * W2, 256], {reference parameter name: gradient});
        `self.dq_all` [L, B * Q, 256] keeps the gradient that enters each layer's output from its
        own heads.  The gradients are views of `self.flat_grad`; `on_ready(end)` as `HeadGrad`.
        `seed_dq` [B * Q, 256] / `seed_dmem` [B, SN, 256] (`BaselineHeadGrad`): a further gradient
        into the last layer's output / a memory gradient to accumulate onto (in place); with the
        default None the launches are the ones this class has always made."""
        if self.st is None:
            raise RuntimeError("backward() needs a forward_from_plan() first")
        g_cls, g_mask, rows, counts = self._check_grads(grads, counts)
        mk = self.masked_keysplit_min_keys
        if mk is not None and (isinstance(mk, bool) or not isinstance(mk, int) or mk < 0):
            raise ValueError("masked_keysplit_min_keys %r: None or an integer >= 0" % (mk,))
        head, w, E, st = self.head, self.head.w, self._E, self.st
        pl, layers = self.dt["pl"], self.dt["layers"]
        B, Q, L = st["B"], self.Q, st["L"]
        N, M, P = L * B * Q, int(rows.shape[0]), pl.HW2
        nc = head.num_classes + 1
        ready = on_ready if on_ready is not None else (lambda end: None)
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
            dme_all = self._zeros(N, 256)
        # ---- mask_embed, cls_embed, post_norm on all rows ----
        dqn = self._mlp3_bwd(dme_all, st["qn"], st["mlp"], "mask_embed", grads_out)
        self._acc(dqn, self._lin_bwd(g_cls.view(N, nc), st["qn"], w["cls_embed.weight"], grads_out,
                                     "cls_embed.weight", "cls_embed.bias"))
        dq_all = self._ln_bwd(dqn, st["q"], "transformer_decoder.post_norm.", grads_out)
        self.dq_all = dq_all.view(L, B * Q, 256)
        ready(self.group_end["heads"])
        # ---- the nine layers, last to first, each layer's own head gradient added in ----
        dmem = self._zeros(B, pl.SN, 256) if seed_dmem is None else seed_dmem
        dqpos_rows = self._zeros(B * Q, 256)
        dx = self.dq_all[L - 1].clone()
        if seed_dq is not None:
            self._acc(dx, seed_dq)
        dx = self._layers_bwd(dx, dqpos_rows, dmem, grads_out, ready, self.dq_all)
        hip.batch_sum(dx, grads_out["query_feat.weight"], B)
        hip.batch_sum(dqpos_rows, grads_out["query_embed.weight"], B)
        ready(self.group_end["query"])
        ready(self.flat_numel)
        return dmem, dMF, grads_out


class BaselineHeadGrad(SegmenterHeadGrad):
    """`SegmenterHeadGrad` plus the relation branch of `CrossHeadBaseline` (baseline.py:363-399): the
    six relation decoder layers over the three memory levels (self-attention first), the two
    two-layer update MLPs on the final queries, the three `F.normalize`s, the two cosine score
    products and `rel_cls_embed` -- every head parameter autograd reaches behind the reference's
    `losses.backward()`, and the complete dmem / dMF:

        tape = BaselineHeadGrad(head); head.forward(...)      (return_all_layers=True)
        out = tape.forward_from_plan(head._last_plan)          # + rel, subject_scores, object_scores
        losses = head.full_losses(..., grads=g)
        dmem, dMF, grads = tape.backward(g, counts=n_b)

    The walk: `rel_cls_embed`; the score products with the normalisations (`pn_cosine_bwd_f32` on
    all three sides: R == Q; d r = the class share, then the subject share, then the object share);
    the update MLPs -> the gradient into the final queries; the relation layers last to first,
    each layer's d K / d V on to the memory, `level_embed` and the layer's own in_proj rows
    256-767; `rel_query_feat` / `rel_query_embed`; then the parent's walk with the final queries'
    share added into layer 8's incoming gradient and the memory / `level_embed` shares summed in.
    The new parameter groups come first in the flat buffer, in completion order.

    `attn_bwd_algo`: the relation layers' cross-attention backward, "keysplit"
    (`pn_mha_bwd_keysplit_f32`: keys split across workgroups, P and dS on chip) or "mha_bwd"
    (`pn_mha_bwd_f32`); the self-attentions always take the latter.  The argmax ids and the four
    output gathers carry no loss term and are not taped."""

    ATTN_BWD_ALGOS = ("keysplit", "mha_bwd")
    REL_KEYS = ("rel", "subject_scores", "object_scores")

    def __init__(self, head, flat=None, base=0):
        if not hasattr(head, "_relation_stage") or head.num_obj_query != head.num_rel_query:
            raise RuntimeError("BaselineHeadGrad needs a CrossHeadBaseline")
        super().__init__(head, flat, base)
        self.rt = None
        # the cross-attentions' backward: "keysplit" (0.61 against 1.67 ms at 16 700 keys, slower at
        # 1 050: 0.21 against 0.14; labnotes R23.4) or "mha_bwd"
        self.attn_bwd_algo = "keysplit"

    @staticmethod
    def param_groups(head):
        groups = [("rel_cls_embed", ["rel_cls_embed.weight", "rel_cls_embed.bias"])]
        for side in ("sub", "obj"):
            groups.append((side + "_query_update", ["%s_query_update.%d.%s" % (side, j, n)
                                                    for j in (2, 0) for n in ("weight", "bias")]))
        for i in reversed(range(head.num_rel_layers)):
            groups.append(("relation_decoder.layers.%d" % i,
                           RelationTailGrad._layer_names("relation_decoder.layers.%d." % i)))
        groups.append(("rel_query", ["rel_query_feat.weight", "rel_query_embed.weight"]))
        return groups + SegmenterHeadGrad.param_groups(head)

    # ------------------------------------------------------------------ forward with a tape
    @torch.no_grad()
    @hip.on_device
    def forward_from_plan(self, pl, with_mask=False, dropout=None):
        """The parent's replay, then the relation stage of `CrossHeadBaseline._relation_stage` taped
        on the exact-fp32 kernels over the plan's `rKp` / `rVp`.  Returns the parent's dict plus
        "rel" [B, R, C + 1], "subject_scores" and "object_scores" [B, R, Q].

        `dropout` (an `FfnDropout`, as `TailTrainer` passes it; default None: the deterministic
        step): the relation decoder's training-mode `ffn_drop`, through the same two `drop.apply`
        sites per layer as `RelationTailGrad`.  With dropout the plan's own relation outputs are the
        eval-mode ones: the TAPED outputs returned here are what the loss must see."""
        self.rt = None
        out = SegmenterHeadGrad.forward_from_plan(self, pl, with_mask)
        head, w, E = self.head, self.head.w, self._E
        B, Q, R = pl.B, self.Q, self.R
        nr = head.num_rel_layers
        if not hasattr(pl, "rKp") or len(pl.rKp) != nr:
            raise RuntimeError("the plan has no relation stage (a CrossHeadBaseline forward)")
        x = E(B * R, 256)
        x.view(B, R, 256).copy_(w["rel_query_feat.weight"].unsqueeze(0).expand(B, R, 256))
        rpos = w["rel_query_embed.weight"]
        scr = E(max(hip.attn_scratch_floats(B, R, n) for n in list(pl.N) + [R]))
        layers = []
        for i in range(nr):
            l = i % 3
            s, x = self._layer_fwd_self_first(
                "relation_decoder.layers.%d." % i, x, rpos, pl.rKp[i].view(B * pl.N[l], 256),
                pl.rVp[i].view(B * pl.N[l], 256), B, R, pl.N[l], head.rel_ffn, scr,
                drop=self._drop_of(dropout, i))
            s["level"] = l
            layers.append(s)
        # query matching (baseline.py:388-399) on the last decoder output BEFORE post_norm
        q = self.dt["q_out"]
        rt = dict(layers=layers, r_out=x, q=q)
        for side in ("sub", "obj"):
            mlp = side + "_query_update"
            h1, e, hat = E(B * Q, 256), E(B * Q, 256), E(B * Q, 256)
            hip.linear(q, w[mlp + ".0.weight"], w[mlp + ".0.bias"], h1, relu=True)
            hip.linear(h1, w[mlp + ".2.weight"], w[mlp + ".2.bias"], e)
            hip.l2normalize(e, hat)
            rt[side] = (h1, e, hat)
        rn = E(B * R, 256)
        hip.l2normalize(x, rn)
        rt["rn"] = rn
        for side, key in (("sub", "subject_scores"), ("obj", "object_scores")):
            sc = E(B, R, Q)
            hip.gemm(rn, rt[side][2], sc, M=R, N=Q, K=256, lda=256, ldw=256, ldc=Q, batch=B,
                     sA=R * 256, sW=Q * 256, sC=R * Q)
            out[key] = sc
        C = w["rel_cls_embed.weight"].shape[0]
        rel = E(B, R, C)
        hip.linear(x, w["rel_cls_embed.weight"], w["rel_cls_embed.bias"], rel.view(B * R, C))
        out["rel"] = rel
        self.rt = rt
        return out

    # ------------------------------------------------------------------ backward
    def _check_rel_grads(self, grads):
        if self.attn_bwd_algo not in self.ATTN_BWD_ALGOS:
            raise ValueError("attn_bwd_algo %r: one of %s" % (self.attn_bwd_algo,
                                                               self.ATTN_BWD_ALGOS,))
        if not isinstance(grads, dict):
            raise ValueError("grads: the dict `full_losses(..., grads={})` fills")
        unknown = sorted(set(grads) - set(("cls", "mask", "mask_rows") + self.REL_KEYS))
        if unknown:
            raise ValueError("grads has unknown keys %s" % unknown)
        B, Q, R = self.st["B"], self.Q, self.R
        C = self.head.w["rel_cls_embed.weight"].shape[0]
        got = []
        for k, shape in zip(self.REL_KEYS, ((B, R, C), (B, R, Q), (B, R, Q))):
            if k not in grads:
                raise ValueError("grads lacks %r (CrossHeadBaseline.full_losses(..., grads={}))" % k)
            t = grads[k]
            if not (torch.is_tensor(t) and t.is_cuda and t.device == self.dev and
                    t.dtype == torch.float32):
                raise ValueError("grads[%r]: an fp32 tensor on %s" % (k, self.dev))
            if tuple(t.shape) != shape:
                raise ValueError("grads[%r] %s does not match the tape's %s"
                                 % (k, tuple(t.shape), shape))
            got.append(t.contiguous())
        return got

    @torch.no_grad()
    @hip.on_device
    def backward(self, grads, on_ready=None, counts=None):
        """`grads`: the six entries `CrossHeadBaseline.full_losses(..., grads={})` fills -- the
        parent's "cls", "mask", "mask_rows" and "rel" [B, R, C + 1], "subject_scores",
        "object_scores" [B, R, Q]; anything else, a wrong shape / dtype / device or a tape without a
        relation stage is refused on the host before any launch.  -> (dmem, dMF, {name: gradient})
        as the parent, now complete; `self.dq_rel` [B * Q, 256] keeps the relation branch's
        gradient into the final queries."""
        if self.st is None or self.rt is None:
            raise RuntimeError("backward() needs a forward_from_plan() with a relation stage first")
        g_rel, g_sub, g_obj = self._check_rel_grads(grads)
        self._check_grads(grads, counts)
        head, w, E, rt = self.head, self.head.w, self._E, self.rt
        pl = self.dt["pl"]
        B, Q, R = pl.B, self.Q, self.R
        ready = on_ready if on_ready is not None else (lambda end: None)
        self._zeroed = False
        g = self._zero_grads()
        # ---- rel_cls_embed ----
        C = g_rel.shape[-1]
        dr = self._lin_bwd(g_rel.view(B * R, C), rt["r_out"], w["rel_cls_embed.weight"], g,
                           "rel_cls_embed.weight", "rel_cls_embed.bias")
        ready(self.group_end["rel_cls_embed"])
        # ---- the two score products and the three normalisations (each backward is linear:
        # d r = class share + subject share + object share, in this order) ----
        dq_rel = self._zeros(B * Q, 256)
        for side, gs in (("sub", g_sub), ("obj", g_obj)):
            h1, e, hat = rt[side]
            dshare, de = E(B * R, 256), E(B * Q, 256)
            hip.cosine_bwd(gs, rt["r_out"], hat, dshare, B, Q, False)
            self._acc(dr, dshare)
            hip.cosine_bwd(gs, e, rt["rn"], de, B, Q, True)
            # ---- the side's update MLP (Linear, ReLU, Linear) -> the final queries ----
            mlp = side + "_query_update"
            d1 = self._lin_bwd(de, h1, w[mlp + ".2.weight"], g, mlp + ".2.weight", mlp + ".2.bias")
            hip.relu_bwd(d1, h1, d1)
            self._acc(dq_rel, self._lin_bwd(d1, rt["q"], w[mlp + ".0.weight"], g,
                                            mlp + ".0.weight", mlp + ".0.bias"))
            ready(self.group_end[mlp])
        self.dq_rel = dq_rel
        # ---- the six relation layers, last to first ----
        keysplit = self.attn_bwd_algo == "keysplit"
        dmem = self._zeros(B, pl.SN, 256)
        drpos_rows = self._zeros(B * R, 256)
        scr = E(max([hip.mha_bwd_scratch_floats(B, R, R)] +
                    ([] if keysplit else [hip.mha_bwd_scratch_floats(B, R, n) for n in pl.N])))
        ks_scr = E(max(hip.mha_bwd_keysplit_scratch_floats(B, R, n) for n in pl.N)) \
            if keysplit else None
        le, dle = w["level_embed.weight"], g["level_embed.weight"]
        dx = dr
        for i in reversed(range(head.num_rel_layers)):
            pre = "relation_decoder.layers.%d." % i
            ac = pre + "attentions.1.attn."
            Wc = w[ac + "in_proj_weight"]
            s = rt["layers"][i]
            l, Nk = s["level"], pl.N[s["level"]]
            dKV = E(B * Nk, 512)                              # columns [dK | dV]
            dx = self._layer_bwd_self_first(pre, s, dx, g, B, R, Nk, scr, drpos_rows,
                                            dKV[:, :256], dKV[:, 256:], keysplit, ks_scr)
            # K = (mem_l + level_embed_l + pe_l) Wk^T + bk, V = (mem_l + level_embed_l) Wv^T + bv
            # (baseline.py:372-384), image by image, as the parent does for its own layers
            for b in range(B):
                mem = pl.X[b, pl.start[l]:pl.start[l] + Nk]
                memk, memv = E(Nk, 256), E(Nk, 256)
                hip.add_periodic(mem, pl.dec_kpos[l], memk)
                hip.add_periodic(mem, le[l:l + 1], memv)
                dmk = self._lin_bwd(dKV[b * Nk:(b + 1) * Nk, :256], memk, Wc[256:512], g,
                                    ac + "in_proj_weight", ac + "in_proj_bias", row0=256)
                dmv = self._lin_bwd(dKV[b * Nk:(b + 1) * Nk, 256:], memv, Wc[512:], g,
                                    ac + "in_proj_weight", ac + "in_proj_bias", row0=512)
                self._acc(dmk, dmv)
                dm = dmem[b, pl.start[l]:pl.start[l] + Nk]
                self._acc(dm, dmk)
                hip.colsum(dmk, dle[l], accumulate=True)
            ready(self.group_end["relation_decoder.layers.%d" % i])
        hip.batch_sum(dx, g["rel_query_feat.weight"], B)
        hip.batch_sum(drpos_rows, g["rel_query_embed.weight"], B)
        ready(self.group_end["rel_query"])
        # ---- the parent's walk on top of the three shares ----
        self._zeroed = True
        try:
            return SegmenterHeadGrad.backward(self, grads, on_ready, counts, seed_dq=dq_rel,
                                              seed_dmem=dmem)
        finally:
            self._zeroed = False


class PSGTr2HeadGrad(SegmenterHeadGrad):
    """The tape of `PSGTrHead2` ("PSGTR on Mask2Former", psgtr_head2.py:288-444): from the six
    entries `PSGTrHead2.triplet_losses(..., grads={})` fills to every head parameter the reference's
    `losses.backward()` reaches behind the pixel decoder (179 tensors), dmem and dMF:

        tape = PSGTr2HeadGrad(head); head.forward(feats, metas)
        out = tape.forward_from_plan(head._last_plan)       # sub, obj, rel, me (, sub_seg, obj_seg)
        losses = head.triplet_losses(..., grads=g)
        dmem, dMF, grads = tape.backward(g, counts=head._tri_loss.last["counts"])

    What differs from the parent: no deep supervision -- only the last layer's output carries loss
    terms -- and ONE head chain over q_all [2 * B * Q, 256].  Rows 0 .. B * Q - 1 are the last
    layer's output (the three class heads and, sic, `obj_mask_embed` -> the returned `sub_seg`);
    rows B * Q .. 2 * B * Q - 1 are the batch-repeated `query_feat` (`obj_mask_embed` -> the stale
    `obj_seg` of the initial forward_head call; module docstring of psgtr_head2.py).  `post_norm` and
    `obj_mask_embed` run on all rows, the class heads on the first half; the two mask products are
    the parent's kernels with L = 2 (subject rows, then object rows shifted by B * Q); the three
    ragged class heads go back in the two launches of `pn_triplet_heads_bwd_f32`
    (csrc/tri_grad.hip).  The second half's gradient lands in `query_feat`'s batch sum.

    `mask_embed.*` and `sub_mask_embed.*` are not in the layout: the first feeds only the detached
    attention masks, the second reaches no output -- autograd leaves both at `grad is None`."""

    KEYS = ("sub", "obj", "rel", "mask_rows", "sub_mask", "obj_mask")

    @staticmethod
    def param_groups(head):
        heads = ["%s_cls_embed.%s" % (h, n) for h in ("sub", "obj", "rel") for n in ("weight", "bias")]
        heads += ["obj_mask_embed.%d.%s" % (j, n) for j in (4, 2, 0) for n in ("weight", "bias")]
        heads += ["transformer_decoder.post_norm.weight", "transformer_decoder.post_norm.bias"]
        return [("heads", heads)] + SegmenterHeadGrad.param_groups(head)[1:]

    # ------------------------------------------------------------------ forward with a tape
    @torch.no_grad()
    @hip.on_device
    def forward_from_plan(self, pl, with_mask=False):
        """Replays the nine masked layers (the attention masks still come from the untrained
        `mask_embed` through `head._head_embed`), then tapes the one head chain.  -> dict(sub, obj
        [1, B, Q, C + 1], rel [1, B, Q, Cr + 1], me [2 * B * Q, 256] and, with `with_mask`, sub_seg /
        obj_seg [1, B, Q, H2, W2]) in buffers of the tape's own."""
        head, w, E = self.head, self.head.w, self._E
        self.st = None
        self._replay_layers(pl)
        B, Q = pl.B, self.Q
        N = B * Q
        q_all = E(2 * N, 256)
        q_all[:N].copy_(self.dt["q_out"])
        q_all[N:].copy_(pl.q0)
        qn, m1, m2, me = E(2 * N, 256), E(2 * N, 256), E(2 * N, 256), E(2 * N, 256)
        hip.layernorm(q_all, w["transformer_decoder.post_norm.weight"],
                      w["transformer_decoder.post_norm.bias"], qn)
        out = {}
        for key, name in (("sub", "sub_cls_embed"), ("obj", "obj_cls_embed"), ("rel", "rel_cls_embed")):
            n = w[name + ".weight"].shape[0]
            out[key] = E(1, B, Q, n)
            hip.linear(qn[:N], w[name + ".weight"], w[name + ".bias"], out[key].view(N, n))
        hip.linear(qn, w["obj_mask_embed.0.weight"], w["obj_mask_embed.0.bias"], m1, relu=True)
        hip.linear(m1, w["obj_mask_embed.2.weight"], w["obj_mask_embed.2.bias"], m2, relu=True)
        hip.linear(m2, w["obj_mask_embed.4.weight"], w["obj_mask_embed.4.bias"], me)
        self.st = dict(q=q_all, qn=qn, mlp=(m1, m2, me), B=B, L=2)
        out["me"] = me
        if with_mask:
            H2, W2 = pl.hw2
            for key, rows in (("sub_seg", me[:N]), ("obj_seg", me[N:])):
                out[key] = E(1, B, Q, H2, W2)
                head._mask_logits(rows, pl, out[key].view(B, Q, pl.HW2))
        return out

    # ------------------------------------------------------------------ backward
    def _check_tri_grads(self, grads, counts):
        st, pl = self.st, self.dt["pl"]
        B, Q = st["B"], self.Q
        w = self.head.w
        if not isinstance(grads, dict):
            raise ValueError("grads: the dict `triplet_losses(..., grads={})` fills")
        unknown = sorted(set(grads) - set(self.KEYS))
        if unknown:
            raise ValueError("grads has unknown keys %s" % unknown)
        for k in self.KEYS:
            if k not in grads:
                raise ValueError("grads lacks %r (PSGTrHead2.triplet_losses(..., grads={}))" % k)
            t = grads[k]
            dt = torch.int64 if k == "mask_rows" else torch.float32
            if not (torch.is_tensor(t) and t.is_cuda and t.device == self.dev and t.dtype == dt):
                raise ValueError("grads[%r]: a %s tensor on %s" % (k, dt, self.dev))
        for k, name in (("sub", "sub_cls_embed"), ("obj", "obj_cls_embed"), ("rel", "rel_cls_embed")):
            shape = (1, B, Q, w[name + ".weight"].shape[0])
            if tuple(grads[k].shape) != shape:
                raise ValueError("grads[%r] %s does not match the tape's %s"
                                 % (k, tuple(grads[k].shape), shape))
        rows = grads["mask_rows"]
        M = int(rows.shape[0])
        for k in ("sub_mask", "obj_mask"):
            g = grads[k]
            if rows.dim() != 1 or g.dim() != 3 or g.shape[0] != M or \
                    (M and tuple(g.shape[1:]) != tuple(pl.hw2)):
                raise ValueError("grads[%r] %s / ['mask_rows'] %s do not match the tape's [M, %d, %d]"
                                 % (k, tuple(g.shape), tuple(rows.shape), pl.hw2[0], pl.hw2[1]))
        if counts is None:
            if B != 1:
                raise ValueError("counts: the matched rows per image (min(Q, R_b)), needed for B > 1")
            counts = [M]
        counts = [int(c) for c in counts]
        if len(counts) != B or min(counts) < 0 or max(counts) > Q or sum(counts) != M:
            raise ValueError("counts %s do not match %d images, %d queries and %d rows"
                             % (counts, B, Q, M))
        return counts

    @torch.no_grad()
    @hip.on_device
    def backward(self, grads, counts=None, on_ready=None):
        """`grads`: "sub", "obj" [1, B, Q, C + 1], "rel" [1, B, Q, Cr + 1], "mask_rows" [M] (rows in
        [0, B * Q), -1 for a failed image) and "sub_mask" / "obj_mask" [M, H2, W2] as
        `PSGTrHead2Loss.loss(..., grads={})` fills them; `counts`: the matched rows per image (the
        loss object's `last["counts"]`; optional for one image).  Nothing is read back from the
        device.  -> (dmem [B, SN, 256], dMF [B, H2 * W2, 256], {reference parameter name:
        gradient}), the gradients views of `self.flat_grad`; `on_ready(end)` as the parent."""
        if self.st is None:
            raise RuntimeError("backward() needs a forward_from_plan() first")
        counts = self._check_tri_grads(grads, counts)
        mk = self.masked_keysplit_min_keys
        if mk is not None and (isinstance(mk, bool) or not isinstance(mk, int) or mk < 0):
            raise ValueError("masked_keysplit_min_keys %r: None or an integer >= 0" % (mk,))
        w, E, st = self.head.w, self._E, self.st
        pl = self.dt["pl"]
        B, Q = st["B"], self.Q
        N, P = B * Q, pl.HW2
        rows = grads["mask_rows"].contiguous()
        M = int(rows.shape[0])
        ready = on_ready if on_ready is not None else (lambda end: None)
        g = self._zero_grads()
        me = st["mlp"][2]
        # ---- the two mask products with L = 2: subject rows, then object rows B * Q further on ----
        table, T = self._table(2, counts)
        gs, go = grads["sub_mask"].contiguous(), grads["obj_mask"].contiguous()
        if M and go.data_ptr() == gs.data_ptr() + 4 * M * P and \
                gs.untyped_storage().data_ptr() == go.untyped_storage().data_ptr():
            G = torch.as_strided(gs, (2 * M, P), (P, 1))          # the two halves of ONE buffer
        else:
            G = torch.cat([gs.view(M, P), go.view(M, P)])
        rows2 = torch.cat([rows, torch.where(rows >= 0, rows + N, rows)])
        dMF = E(B, P, 256)
        hip.mask_feature_grad(G, me, rows2, table, T, dMF)
        if M:
            dme = E(2 * M, 256)
            hip.mask_embed_grad(G, pl.MF.view(B, P, 256), rows2, table, T, dme,
                                E(hip.mask_embed_grad_scratch_floats(T, P)))
            dme_all = E(2 * N, 256)             # (a matched row appears once; failed rows match none)
            hip.scatter_rows_add(dme, rows2, dme_all, 1, 2 * N, 2 * M, 256)
        else:
            dme_all = self._zeros(2 * N, 256)
        # ---- obj_mask_embed on all rows, the three class heads on the first half, post_norm ----
        dqn = self._mlp3_bwd(dme_all, st["qn"], st["mlp"], "obj_mask_embed", g)
        hip.tri_heads_bwd(
            grads["sub"].contiguous().view(N, -1), grads["obj"].contiguous().view(N, -1),
            grads["rel"].contiguous().view(N, -1), st["qn"][:N], w["sub_cls_embed.weight"],
            w["obj_cls_embed.weight"], w["rel_cls_embed.weight"], dqn[:N],
            g["sub_cls_embed.weight"], g["sub_cls_embed.bias"], g["obj_cls_embed.weight"],
            g["obj_cls_embed.bias"], g["rel_cls_embed.weight"], g["rel_cls_embed.bias"], add=True)
        dq_all = self._ln_bwd(dqn, st["q"], "transformer_decoder.post_norm.", g)
        self.dq_all = dq_all.view(2, N, 256)
        ready(self.group_end["heads"])
        # ---- the nine layers, last to first, from the first half; no deep supervision ----
        dmem = self._zeros(B, pl.SN, 256)
        dqpos_rows = self._zeros(N, 256)
        dx = self._layers_bwd(self.dq_all[0].clone(), dqpos_rows, dmem, g, ready)
        hip.batch_sum(dx, g["query_feat.weight"], B)
        hip.batch_sum(self.dq_all[1], g["query_feat.weight"], B, accumulate=True)   # the stale masks
        hip.batch_sum(dqpos_rows, g["query_embed.weight"], B)
        ready(self.group_end["query"])
        ready(self.flat_numel)
        return dmem, dMF, g


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
    call to call, as `PixelDecoderGrad.backward`'s results always have -- unless the tape's
    `deterministic` attribute (inherited from the parent) is set: then the walk runs
    `pn_msda_bwd_det_f32` and all of it is bitwise reproducible."""

    BRANCH_GROUPS = [
        ("mask_feature", [PixelDecoderGrad.PD + "mask_feature." + n for n in ("weight", "bias")]),
        ("output_convs.0", [PixelDecoderGrad.PD + "output_convs.0." + n
                            for n in ("conv.weight", "gn.weight", "gn.bias")]),
        ("lateral_convs.0", [PixelDecoderGrad.PD + "lateral_convs.0." + n
                             for n in ("conv.weight", "gn.weight", "gn.bias")])]

    def __init__(self, head, flat=None, base=0):
        super().__init__(head, flat, base)
        self.dgrad_algo = "winograd4"   # the 3x3's data gradient: "winograd4" or "direct"

    @staticmethod
    def param_groups(head):
        return list(SegPixelDecoderGrad.BRANCH_GROUPS) + PixelDecoderGrad.param_groups(head)

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
