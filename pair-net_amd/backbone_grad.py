"""Backward of the backbones' trainable parts, taped and differentiated from the gradients of
their output maps (what pixel_grad.py's `PixelDecoderGrad.backward` returns): `BackboneGrad` (mmdet
ResNet-50 / -101 stages 2-4 under frozen BatchNorm), `SwinBackboneGrad` (the Swin backbone's last
stage, `frozen_stages=3`) and `SwinStagesGrad` (every trainable Swin stage with its patch merging
and the patch embedding)."""
import torch

from . import hip
from .tape import Tape

__all__ = ["BackboneGrad", "SwinBackboneGrad", "SwinStagesGrad"]


class BackboneGrad(Tape):
    """The backbone's trainable part -- mmdet ResNet-50 / -101 stages 2-4 (`frozen_stages=1`: stem
    and layer1 fixed; BatchNorm frozen, `norm_eval`: configs/mask2former/pairnet.py:9-19) -- taped
    and differentiated from C2 (layer1's output) to C3 / C4 / C5:

        tape = BackboneGrad(det.backbone)
        c3, c4, c5 = tape.forward(c2)                  # channel-last [B, h, w, C] maps
        grads = tape.backward(d_c3, d_c4, d_c5)        # [B, C, h, w], e.g. PixelDecoderGrad's dfeats

    Frozen BatchNorm is folded into the convolutions (W' = W gamma / sqrt(var + eps), as the
    inference path does); the gradient of the un-folded weight is the folded one's times the same
    per-channel factor.  1x1 convolutions are linear layers over pixels (`pn_gemm_f32` on
    transposed operands), the 3x3 convolutions' data gradient is the forward implicit-GEMM kernel on
    the tap-reversed, channel-swapped weight (over the zero-dilated gradient map for the stride-2
    layers), their weight gradient `pn_conv_wgrad_f32` (MFMA outer products over pixels).  The taped
    forward uses the direct implicit-GEMM convolution where inference uses Winograd (same values to
    ~1e-5).  Gradients are named like the backbone's state dict (`layer3.4.conv2.weight`)."""

    def __init__(self, backbone, flat=None, base=0):
        if getattr(backbone, "groups", 1) != 1:     # (ResNeXtHip subclasses the ResNet)
            raise NotImplementedError("ResNeXt backbone: forward only")
        super().__init__(backbone, flat, base)
        self.backbone = backbone
        P = backbone._params
        self.bn_scale, self.bn_scale64 = {}, {}
        for n in self.layout:                      # conv name -> gamma / sqrt(var + eps)
            conv = n[:-len(".weight")]
            bn = conv.replace("conv", "bn") if "downsample" not in conv else conv[:-1] + "1"
            sc = P[bn + ".weight"].double() / torch.sqrt(P[bn + ".running_var"].double() + 1e-5)
            self.bn_scale[n] = sc.float().to(self.dev)
            self.bn_scale64[n] = sc.to(self.dev)

    @staticmethod
    def param_groups(backbone):
        groups = []
        stages = list(enumerate(backbone.stages))
        for i, (planes, blocks) in reversed(stages[1:]):
            for b in reversed(range(blocks)):
                p = "layer%d.%d." % (i + 1, b)
                names = [p + "conv3.weight", p + "conv2.weight", p + "conv1.weight"]
                if b == 0:
                    names.append(p + "downsample.0.weight")
                groups.append((p[:-1], names))
        return groups

    @torch.no_grad()
    @hip.on_device
    def forward(self, c2):
        bb, w, E = self.backbone, self.backbone.w, self._E
        B, cin, h, wd = c2.shape
        x = c2.permute(0, 2, 3, 1).contiguous()             # channel-last rows
        blocks_t, outs = [], []
        for i, (planes, blocks) in list(enumerate(bb.stages))[1:]:
            for b in range(blocks):
                p = "layer%d.%d." % (i + 1, b)
                stride = 2 if b == 0 else 1
                hi, wi = h, wd
                if stride == 2:
                    h, wd = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
                s = dict(p=p, x=x, cin=cin, planes=planes, stride=stride, hi=hi, wi=wi, h=h, w=wd)
                s["t1"] = E(B, hi, wi, planes)
                hip.linear(x.view(-1, cin), w[p + "conv1.w"], w[p + "conv1.b"],
                           s["t1"].view(-1, planes), relu=True)
                s["t2"] = E(B, h, wd, planes)
                hip.conv2d_ex(s["t1"], w[p + "conv2.w"], w[p + "conv2.b"], None, s["t2"], B, hi, wi,
                              planes, planes, 3, 3, stride, 1, relu=True)
                if b == 0:
                    idt = E(B, h, wd, planes * 4)
                    hip.conv2d_ex(x, w[p + "downsample.0.w"], w[p + "downsample.0.b"], None, idt, B,
                                  hi, wi, cin, planes * 4, 1, 1, stride, 0)
                else:
                    idt = x
                s["out"] = E(B, h, wd, planes * 4)
                hip.linear(s["t2"].view(-1, planes), w[p + "conv3.w"], w[p + "conv3.b"],
                           s["out"].view(-1, planes * 4), res=idt.view(-1, planes * 4),
                           relu_after=True)
                x, cin = s["out"], planes * 4
                blocks_t.append(s)
            outs.append(x)
        self.t = dict(B=B, blocks=blocks_t)
        return tuple(outs)

    def _conv3x3_bwd(self, s, d_t2, grads, B):
        """d_t2 [B, h, w, planes] (pre-ReLU) -> d t1 (post-ReLU input of the 3x3), + its weight."""
        w, E = self.backbone.w, self._E
        p, planes, stride = s["p"], s["planes"], s["stride"]
        hi, wi, h, wd = s["hi"], s["wi"], s["h"], s["w"]
        rows_per = max(1, min(h, 8))
        chunks = B * ((h + rows_per - 1) // rows_per)
        part = E(chunks, planes * 9 * planes)
        hip.conv_wgrad(d_t2, s["t1"], part, B, hi, wi, h, wd, planes, planes, 3, stride, 1, rows_per)
        dwp = E(planes * 9 * planes)                          # [co][tap][ci]: the packed layout
        hip.colsum(part, dwp)
        g = grads[p + "conv2.weight"]
        g.copy_(dwp.view(planes, 3, 3, planes).permute(0, 3, 1, 2))      # -> [co][ci][3][3]
        hip.scale_rows(g, self.bn_scale[p + "conv2.weight"])
        wb = E(planes * 9 * planes)
        hip.conv_weight_bwd_layout(w[p + "conv2.w"], wb, planes, 9, planes)
        d_t1 = E(B, hi, wi, planes)
        if stride == 1:
            src = d_t2
        else:
            src = E(B, hi, wi, planes)
            hip.dilate2(d_t2, src, B, hi, wi, h, wd, planes)
        hip.conv2d_ex(src, wb.view(planes, 9 * planes), None, None, d_t1, B, hi, wi, planes, planes,
                      3, 3, 1, 1)
        return d_t1

    @torch.no_grad()
    @hip.on_device
    def backward(self, d_c3, d_c4, d_c5, on_ready=None):
        if self.t is None:
            raise RuntimeError("backward() needs a forward() first")
        w, E, t = self.backbone.w, self._E, self.t
        B = t["B"]
        ready = on_ready if on_ready is not None else (lambda end: None)
        grads = self._zero_grads()
        nhwc = lambda g: g.to(self.dev, torch.float32).permute(0, 2, 3, 1).contiguous()
        stage_grads = {2: nhwc(d_c3), 3: nhwc(d_c4), 4: nhwc(d_c5)}     # by layer number
        dx = None
        for s in reversed(t["blocks"]):
            p, planes, cin, stride = s["p"], s["planes"], s["cin"], s["stride"]
            hi, wi, h, wd = s["hi"], s["wi"], s["h"], s["w"]
            layer, blk = int(p[5]), int(p[7:-1])
            last_of_stage = blk == self.backbone.stages[layer - 1][1] - 1
            if last_of_stage:                      # a stage's output also feeds the pixel decoder
                g = stage_grads[layer]
                if dx is not None:
                    self._acc(g, dx)
                dx = g
            dy = E(B, h, wd, planes * 4)
            hip.relu_bwd(dx, s["out"], dy)         # ReLU after the shortcut
            # conv3 (1x1) + BN
            d_t2 = self._lin_bwd(dy.view(-1, planes * 4), s["t2"].view(-1, planes), w[p + "conv3.w"],
                                 grads, p + "conv3.weight", None)
            hip.scale_rows(grads[p + "conv3.weight"], self.bn_scale[p + "conv3.weight"])
            hip.relu_bwd(d_t2, s["t2"].view(-1, planes), d_t2)
            d_t1 = self._conv3x3_bwd(s, d_t2.view(B, h, wd, planes), grads, B)
            hip.relu_bwd(d_t1, s["t1"], d_t1)
            first = layer == 2 and blk == 0        # its input is the frozen layer1's output
            dxin = self._lin_bwd(d_t1.view(-1, planes), s["x"].view(-1, cin), w[p + "conv1.w"], grads,
                                 p + "conv1.weight", None, need_dx=not first)
            hip.scale_rows(grads[p + "conv1.weight"], self.bn_scale[p + "conv1.weight"])
            if blk == 0:                           # projection shortcut (1x1, stride s)
                xs = s["x"]
                if stride == 2:
                    xs = E(B, h, wd, cin)
                    hip.subsample2(s["x"], xs, B, hi, wi, h, wd, cin)
                dxs = self._lin_bwd(dy.view(-1, planes * 4), xs.view(-1, cin),
                                    w[p + "downsample.0.w"], grads, p + "downsample.0.weight", None,
                                    need_dx=not first)
                hip.scale_rows(grads[p + "downsample.0.weight"],
                               self.bn_scale[p + "downsample.0.weight"])
                if not first:
                    if stride == 2:
                        hip.dilate2(dxs, dxin, B, hi, wi, h, wd, cin, accumulate=True)
                    else:
                        self._acc(dxin, dxs)
            else:                                  # identity shortcut
                self._acc(dxin, dy.view(-1, planes * 4))
            dx = None if first else dxin.view(B, hi, wi, cin)
            ready(self.group_end[p[:-1]])
        ready(self.flat_numel)
        return grads


class SwinBackboneGrad(Tape):
    """The Swin backbone's trainable part -- the two blocks of the last stage and its output norm
    (configs/mask2former/pairnet_swinb.py:201-240, `frozen_stages=3`: mmdet's `_freeze_stages`
    fixes patch_embed, stages 0-2 with their patch merging, and norm0-norm2) -- taped and
    differentiated from the stage-4 input tokens to C5:

        tape = SwinBackboneGrad(swin)             # swin.frozen_stages must be 3
        x4 = tape.stage_input()                   # [B, h4, w4, C4] of the backbone's last forward
        c5 = tape.forward(x4, keep=None)          # channel-last [B, h4, w4, C4]
        grads = tape.backward(d_c5)               # d_c5 [B, C4, h4, w4], e.g. PixelDecoderGrad's dfeats[0]

    Per block: norm1 -> qkv -> (shifted-)window attention -> proj (+ residual) -> norm2 -> FFN
    Linear -> GELU -> FFN Linear (+ residual), on the exact-fp32 kernels whatever
    `swin.gemm_arithmetic` says.  The attention backward (`pn_window_attention_bwd_f32`) returns
    the qkv gradient over the PADDED token grid: the reference pads the normalised map before the
    qkv Linear, so the padding tokens' gradient belongs to `qkv.bias`.  `keep` [blocks, 2, B]:
    mmdet's DropPath as per-image scale factors of the (attention, FFN) residual branches (0 or
    1 / (1 - p)), None for none.  Gradients are named like the backbone's state dict; the bias
    table's in the reference layout [(2ws-1)^2, heads]."""

    BLOCK_PARAMS = ("norm1.weight", "norm1.bias", "attn.w_msa.relative_position_bias_table",
                    "attn.w_msa.qkv.weight", "attn.w_msa.qkv.bias", "attn.w_msa.proj.weight",
                    "attn.w_msa.proj.bias", "norm2.weight", "norm2.bias", "ffn.layers.0.0.weight",
                    "ffn.layers.0.0.bias", "ffn.layers.1.weight", "ffn.layers.1.bias")
    EPS = 1e-5

    def __init__(self, backbone, flat=None, base=0):
        if getattr(backbone, "frozen_stages", -1) != len(backbone.depths) - 1:
            raise NotImplementedError("SwinBackboneGrad trains the last stage only (frozen_stages=%d, "
                                      "the reference's config); got frozen_stages=%s"
                                      % (len(backbone.depths) - 1,
                                         getattr(backbone, "frozen_stages", -1)))
        S = len(backbone.depths) - 1
        if S not in backbone.out_indices:
            raise NotImplementedError("the last stage must be an output stage (norm%d)" % S)
        super().__init__(backbone, flat, base)
        self.backbone, self.S = backbone, S
        self.C, self.heads, self.ws = backbone.num_features[S], backbone.num_heads[S], backbone.ws

    @staticmethod
    def param_groups(backbone):
        S = len(backbone.depths) - 1
        groups = [("norm%d" % S, ["norm%d.weight" % S, "norm%d.bias" % S])]
        for j in reversed(range(backbone.depths[S])):
            p = "stages.%d.blocks.%d." % (S, j)
            groups.append((p[:-1], [p + n for n in SwinBackboneGrad.BLOCK_PARAMS]))
        return groups

    @torch.no_grad()
    @hip.on_device
    def stage_input(self):
        """The last stage's input tokens [B, h, w, C] of the backbone's most recent forward: its
        plan's patch-merge buffer still holds the merged rows of the stage before (the last stage
        has no patch merging), so the frozen reduction GEMM is run on them once more."""
        bb = self.backbone
        pl = getattr(bb, "_last_plan", None)
        if pl is None:
            raise RuntimeError("stage_input() needs a forward of the backbone first")
        B, S = bb._last_batch, self.S
        C2 = bb.num_features[S - 1]
        h, wd = pl.hw[S]
        n = B * h * wd
        x4 = self._E(B, h, wd, self.C)
        hip.linear(pl.merged[:n * 4 * C2].view(n, 4 * C2),
                   bb.w["stages.%d.downsample.reduction.weight" % (S - 1)], None, x4.view(n, self.C),
                   scratch=pl.scratch)
        return x4

    def _branch(self, out, x, keep):
        """out (the branch's rows) <- x + keep[image] * out"""
        if keep is not None:
            hip.scale_rows(out, keep)
        hip.add_periodic(out, x, out)

    def _block_fwd(self, p, x, B, h, wd, C, nh, shift, keep):
        """One SwinBlock `p` on the token rows x [B*h*wd, C] with a tape: (saved tensors, output
        rows).  `keep` [2, B]: the block's DropPath factors (attention, FFN branch) or None."""
        w, E, ws = self.backbone.w, self._E, self.ws
        n, F = B * h * wd, int(self.backbone.mlp_ratio * C)
        s = dict(x=x, shift=shift)
        s["xn1"] = E(n, C)
        hip.layernorm_rows(x, w[p + "norm1.weight"], w[p + "norm1.bias"], s["xn1"], self.EPS)
        s["qkv"] = E(n, 3 * C)
        hip.linear(s["xn1"], w[p + "attn.w_msa.qkv.weight"], w[p + "attn.w_msa.qkv.bias"], s["qkv"])
        s["ao"] = E(n, C)
        hip.window_attention(s["qkv"], w[p + "attn.w_msa.qkv.bias"],
                             w[p + "attn.w_msa.relative_position_bias_table"], s["ao"], B, h, wd,
                             C, nh, ws, s["shift"])
        s["x1"] = E(n, C)
        if keep is None:
            hip.linear(s["ao"], w[p + "attn.w_msa.proj.weight"], w[p + "attn.w_msa.proj.bias"],
                       s["x1"], res=x)
        else:
            hip.linear(s["ao"], w[p + "attn.w_msa.proj.weight"], w[p + "attn.w_msa.proj.bias"],
                       s["x1"])
            self._branch(s["x1"], x, keep[0])
        s["xn2"] = E(n, C)
        hip.layernorm_rows(s["x1"], w[p + "norm2.weight"], w[p + "norm2.bias"], s["xn2"], self.EPS)
        s["pre"], s["hid"] = E(n, F), E(n, F)
        hip.linear(s["xn2"], w[p + "ffn.layers.0.0.weight"], w[p + "ffn.layers.0.0.bias"], s["pre"])
        hip.gelu(s["pre"], s["hid"])
        x = E(n, C)
        if keep is None:
            hip.linear(s["hid"], w[p + "ffn.layers.1.weight"], w[p + "ffn.layers.1.bias"], x,
                       res=s["x1"])
        else:
            hip.linear(s["hid"], w[p + "ffn.layers.1.weight"], w[p + "ffn.layers.1.bias"], x)
            self._branch(x, s["x1"], keep[1])
        return s, x

    @torch.no_grad()
    @hip.on_device
    def forward(self, x4, keep=None):
        bb, w, E = self.backbone, self.backbone.w, self._E
        if not (x4.is_cuda and x4.dtype == torch.float32 and x4.dim() == 4 and x4.shape[3] == self.C):
            raise RuntimeError("x4 must be a [B, h, w, %d] fp32 device tensor" % self.C)
        B, h, wd, C = x4.shape
        n, S, ws, nh = B * h * wd, self.S, self.ws, self.heads
        depth = bb.depths[S]
        if keep is not None:
            keep = keep.to(self.dev, torch.float32).contiguous()
            if tuple(keep.shape) != (depth, 2, B):
                raise ValueError("keep must be [%d blocks, 2 branches, B=%d]" % (depth, B))
        x = x4.reshape(n, C).clone()
        blocks = []
        for j in range(depth):
            s, x = self._block_fwd("stages.%d.blocks.%d." % (S, j), x, B, h, wd, C, nh,
                                   0 if j % 2 == 0 else ws // 2,
                                   None if keep is None else keep[j])
            blocks.append(s)
        c5 = E(B, h, wd, C)
        hip.layernorm_rows(x, w["norm%d.weight" % S], w["norm%d.bias" % S], c5.view(n, C), self.EPS)
        self.t = dict(B=B, h=h, w=wd, blocks=blocks, out=x, keep=keep)
        return c5

    def _lnr_bwd(self, dy, x, prefix, grads, acc=None):
        """LayerNorm (any width) backward from its saved input; accumulates d weight / d bias;
        returns dx (+ acc)."""
        dx, gx = self._E(*x.shape), self._E(*x.shape)
        hip.layernorm_rows_bwd(dy, x, self.backbone.w[prefix + "weight"], dx, gx, self.EPS)
        hip.colsum(gx, grads[prefix + "weight"], accumulate=True)
        hip.colsum(dy, grads[prefix + "bias"], accumulate=True)
        if acc is not None:
            self._acc(dx, acc)
        return dx

    def _scaled(self, d, keep):
        if keep is None:
            return d
        out = d.clone()
        hip.scale_rows(out, keep)
        return out

    def _block_bwd(self, p, s, dx, grads, B, h, wd, C, nh, keep):
        """Backward of `_block_fwd`: dx [B*h*wd, C] the gradient of the block's output rows, `s` its
        saved tensors; accumulates the block's parameter gradients, returns d of its input rows."""
        w, E, ws = self.backbone.w, self._E, self.ws
        n = B * h * wd
        hp, wp = -(-h // ws) * ws, -(-wd // ws) * ws
        nrel = (2 * ws - 1) ** 2
        a = p + "attn.w_msa."
        # x_out = x1 + keep * FFN(norm2(x1))
        dbr = self._scaled(dx, None if keep is None else keep[1])
        dhid = self._lin_bwd(dbr, s["hid"], w[p + "ffn.layers.1.weight"], grads,
                             p + "ffn.layers.1.weight", p + "ffn.layers.1.bias")
        hip.gelu_bwd(dhid, s["pre"], dhid)
        dxn2 = self._lin_bwd(dhid, s["xn2"], w[p + "ffn.layers.0.0.weight"], grads,
                             p + "ffn.layers.0.0.weight", p + "ffn.layers.0.0.bias")
        del dhid
        dx1 = self._lnr_bwd(dxn2, s["x1"], p + "norm2.", grads, acc=dx)
        # x1 = x + keep * proj(W-MSA(norm1(x)))
        dbr = self._scaled(dx1, None if keep is None else keep[0])
        dao = self._lin_bwd(dbr, s["ao"], w[a + "proj.weight"], grads, a + "proj.weight",
                            a + "proj.bias")
        dqkv = E(B * hp * wp, 3 * C)
        part = E(hip.window_partials_rows(B, h, wd, ws), nh * nrel)
        hip.window_attention_bwd(s["qkv"], w[a + "qkv.bias"], w[a + "relative_position_bias_table"],
                                 dao, dqkv, part, B, h, wd, C, nh, ws, s["shift"], out=s["ao"])
        dtab = E(nh, nrel)
        hip.colsum(part, dtab.view(-1))
        hip.transpose(dtab, grads[a + "relative_position_bias_table"])    # -> [(2ws-1)^2, heads]
        hip.colsum(dqkv, grads[a + "qkv.bias"], accumulate=True)         # padding rows included
        dq_real = dqkv if (hp, wp) == (h, wd) else \
            dqkv.view(B, hp, wp, 3 * C)[:, :h, :wd].reshape(n, 3 * C)
        dxn1 = self._lin_bwd(dq_real, s["xn1"], w[a + "qkv.weight"], grads, a + "qkv.weight", None)
        return self._lnr_bwd(dxn1, s["x"], p + "norm1.", grads, acc=dx1)

    @torch.no_grad()
    @hip.on_device
    def backward(self, d_c5, on_ready=None, need_dx=False):
        """d_c5 [B, C, h, w] (any memory format) -> {name: gradient} (views of the flat buffer,
        valid until the next backward); with `need_dx` also d x4 [B, h, w, C]."""
        if self.t is None:
            raise RuntimeError("backward() needs a forward() first")
        bb, w, E, t = self.backbone, self.backbone.w, self._E, self.t
        B, h, wd, S, ws, nh = t["B"], t["h"], t["w"], self.S, self.ws, self.heads
        C, n, keep = self.C, B * h * wd, t["keep"]
        ready = on_ready if on_ready is not None else (lambda end: None)
        grads = self._zero_grads()
        dc = d_c5.to(self.dev, torch.float32).permute(0, 2, 3, 1).contiguous().view(n, C)
        dx = self._lnr_bwd(dc, t["out"], "norm%d." % S, grads)
        ready(self.group_end["norm%d" % S])
        for j in reversed(range(bb.depths[S])):
            p = "stages.%d.blocks.%d." % (S, j)
            dx = self._block_bwd(p, t["blocks"][j], dx, grads, B, h, wd, C, nh,
                                 None if keep is None else keep[j])
            ready(self.group_end[p[:-1]])
        ready(self.flat_numel)
        if need_dx:
            return grads, dx.view(B, h, wd, C)
        return grads


class SwinStagesGrad(SwinBackboneGrad):
    """The Swin backbone with `frozen_stages` in {-1, 0, 1, 2} (configs/deformable_detr/
    cross_swinb_vg.py:202-226 trains every stage, `frozen_stages=-1`): taped from the IMAGE and
    differentiated from C2 ... C5 back through every trainable stage, its patch merging and -- with
    `frozen_stages=-1` -- the patch embedding:

        tape = SwinStagesGrad(swin)
        c2, c3, c4, c5 = tape.forward(img, keep=None)      # channel-last [B, h, w, C]
        grads = tape.backward(d_c3, d_c4, d_c5)            # [B, C, h, w] each (d_c2= optional)

    mmdet's `_freeze_stages`: any `frozen_stages >= 0` fixes patch_embed; stages[i - 1] (blocks and
    downsample) and norm{i - 1} are fixed for 1 <= i <= frozen_stages.  The frozen front runs on the
    same exact-fp32 kernels without a tape.  Per trainable stage, walking backward: the gradient of
    the stage's input tokens goes through the patch merging before it -- the reduction Linear
    (`_lin_bwd`), then `pn_patch_merge_ln_bwd_f32`, which ADDS its dx to the share the stage
    output's own norm{i} has already written -- then through the stage's blocks in reverse
    (`_block_bwd`, shared with SwinBackboneGrad).  The patch embedding's weight gradient is
    dY^T cols over `pn_patch_im2col4_f32`'s rows (the image needs no gradient).

    `keep` [sum(depths), 2, B]: DropPath factors of EVERY block (rates linspace(0, drop_path_rate,
    sum(depths)) as mmdet); the rows of frozen stages are ignored (mmdet keeps frozen modules in
    eval mode).  `norm0` is in the layout whenever stage 0 trains but gets a gradient only with
    `d_c2=` (CrossHead2's loss does not reach C2: `NO_GRAD_GROUPS`)."""

    NO_GRAD_GROUPS = ("norm0",)      # zero gradient unless d_c2 is supplied (TailTrainer: lr 0, wd 0)

    def __init__(self, backbone, flat=None, base=0):
        nst = len(backbone.depths)
        f = getattr(backbone, "frozen_stages", -1)
        if not -1 <= f < nst - 1:
            raise NotImplementedError("SwinStagesGrad takes frozen_stages in -1 .. %d (%d: "
                                      "SwinBackboneGrad); got %s" % (nst - 2, nst - 1, f))
        if tuple(backbone.out_indices) != tuple(range(nst)):
            raise NotImplementedError("every stage must be an output stage (out_indices=%s)"
                                      % (tuple(range(nst)),))
        Tape.__init__(self, backbone, flat, base)      # (not the parent's: it takes frozen_stages=3)
        self.backbone = backbone
        self.S, self.ws, self.first = nst - 1, backbone.ws, max(f, 0)
        self.train_embed = f < 0

    @staticmethod
    def param_groups(backbone):
        nst = len(backbone.depths)
        f = getattr(backbone, "frozen_stages", -1)
        groups = []
        for i in reversed(range(max(f, 0), nst)):
            if i < nst - 1:
                d = "stages.%d.downsample." % i
                groups.append((d + "reduction", [d + "reduction.weight"]))
            groups.append(("norm%d" % i, ["norm%d.weight" % i, "norm%d.bias" % i]))
            if i < nst - 1:
                groups.append((d + "norm", [d + "norm.weight", d + "norm.bias"]))
            for j in reversed(range(backbone.depths[i])):
                p = "stages.%d.blocks.%d." % (i, j)
                groups.append((p[:-1], [p + n for n in SwinBackboneGrad.BLOCK_PARAMS]))
        if f < 0:
            groups.append(("patch_embed", ["patch_embed.norm.weight", "patch_embed.norm.bias",
                                           "patch_embed.projection.weight",
                                           "patch_embed.projection.bias"]))
        return groups

    def stage_input(self):
        raise NotImplementedError("SwinStagesGrad.forward starts from the image")

    @torch.no_grad()
    @hip.on_device
    def forward(self, img, keep=None):
        bb, w, E = self.backbone, self.backbone.w, self._E
        if not (img.is_cuda and img.dtype == torch.float32 and img.dim() == 4 and img.shape[1] == 3):
            raise RuntimeError("img must be a [B, 3, H, W] fp32 device tensor")
        img = img.contiguous()
        B, _, H, W = img.shape
        nblk, ws = sum(bb.depths), self.ws
        if keep is not None:
            keep = keep.to(self.dev, torch.float32).contiguous()
            if tuple(keep.shape) != (nblk, 2, B):
                raise ValueError("keep must be [%d blocks, 2 branches, B=%d]" % (nblk, B))
        h, wd = -(-H // 4), -(-W // 4)
        C = bb.num_features[0]
        n = B * h * wd
        cols, proj, x = E(n, 64), E(n, C), E(n, C)
        hip.patch_im2col4(img, cols, B, H, W)
        hip.linear(cols, w["patch_embed.projection.weight"], w["patch_embed.projection.bias"], proj)
        hip.layernorm_rows(proj, w["patch_embed.norm.weight"], w["patch_embed.norm.bias"], x, self.EPS)
        embed = dict(cols=cols, proj=proj) if self.train_embed else None
        del cols, proj
        stages, outs, blk0 = [], [], 0
        for i, (depth, nh) in enumerate(zip(bb.depths, bb.num_heads)):
            C, n = bb.num_features[i], B * h * wd
            taped = i >= self.first
            st = dict(h=h, w=wd, C=C, nh=nh, blk0=blk0, blocks=[])
            for j in range(depth):
                kj = keep[blk0 + j] if (keep is not None and taped) else None
                s, x = self._block_fwd("stages.%d.blocks.%d." % (i, j), x, B, h, wd, C, nh,
                                       0 if j % 2 == 0 else ws // 2, kj)
                if taped:
                    st["blocks"].append(s)
                del s
            blk0 += depth
            c = E(B, h, wd, C)
            hip.layernorm_rows(x, w["norm%d.weight" % i], w["norm%d.bias" % i], c.view(n, C), self.EPS)
            outs.append(c)
            if taped:
                st["out"] = x
            if i < self.S:
                p = "stages.%d.downsample." % i
                h2, w2 = -(-h // 2), -(-wd // 2)
                n2 = B * h2 * w2
                mg, xn = E(n2, 4 * C), E(n2, 2 * C)
                hip.patch_merge_ln(x, w[p + "norm.weight"], w[p + "norm.bias"], mg, B, h, wd, C, self.EPS)
                hip.linear(mg, w[p + "reduction.weight"], None, xn)
                if taped:
                    st["mg"] = mg                 # the reduction Linear's input (its dW)
                x, h, wd = xn, h2, w2
                del mg, xn
            stages.append(st if taped else None)
        self.t = dict(B=B, H=H, W=W, stages=stages, embed=embed, keep=keep)
        return tuple(outs)

    @staticmethod
    def _unfold_order(g, C):
        """[..., 4C] neighbour-major ((row*2+col)*C + c, the packed order) -> nn.Unfold order
        (c*4 + row*2+col, the reference parameter's)."""
        return g.reshape(*g.shape[:-1], 4, C).transpose(-1, -2).reshape(g.shape)

    def _reduction_bwd(self, i, st, dxin, grads, ready):
        """Backward of stage i's patch-merging Linear: dxin [n2, 2C] (d of the next stage's input
        tokens) -> (parameter prefix, d of the merged, normalised rows [n2, 4C])."""
        w, C = self.backbone.w, st["C"]
        p = "stages.%d.downsample." % i
        # reduction Linear (no bias); the packed weight and hence dW have neighbour-major columns
        tmp = {"w": self._zeros(2 * C, 4 * C)}
        dmg = self._lin_bwd(dxin, st["mg"], w[p + "reduction.weight"], tmp, "w", None)
        grads[p + "reduction.weight"].copy_(self._unfold_order(tmp["w"], C))
        ready(self.group_end[p + "reduction"])
        return p, dmg

    def _patch_embed_bwd(self, dx0, grads):
        """dx0 [B*h*w, C]: d of the patch embedding's output tokens -> its four parameter gradients
        (the image needs none)."""
        w, em, C = self.backbone.w, self.t["embed"], self.backbone.num_features[0]
        dproj = self._lnr_bwd(dx0, em["proj"], "patch_embed.norm.", grads)
        # dW = dY^T cols over the 64-column im2col rows (the last 16 zero) -> [C][3][4][4]
        tmp = {"w": self._zeros(C, 64),
               "b": grads["patch_embed.projection.bias"]}
        self._lin_bwd(dproj, em["cols"], w["patch_embed.projection.weight"], tmp, "w", "b",
                      need_dx=False)
        grads["patch_embed.projection.weight"].view(C, 48).copy_(tmp["w"][:, :48])

    @torch.no_grad()
    @hip.on_device
    def backward(self, d_c3, d_c4, d_c5, d_c2=None, on_ready=None):
        """d_c* [B, C, h, w] (any memory format) -> {state-dict name: gradient} (views of the flat
        buffer, valid until the next backward).  A frozen stage's map gradient is ignored."""
        if self.t is None:
            raise RuntimeError("backward() needs a forward() first")
        bb, w, E, t = self.backbone, self.backbone.w, self._E, self.t
        B, keep = t["B"], t["keep"]
        ready = on_ready if on_ready is not None else (lambda end: None)
        grads = self._zero_grads()
        d_maps = [d_c2, d_c3, d_c4, d_c5]
        dxin = None                                # d of the tokens entering the stage above
        for i in reversed(range(self.first, self.S + 1)):
            st = t["stages"][i]
            h, wd, C, nh = st["h"], st["w"], st["C"], st["nh"]
            n = B * h * wd
            dmg = None
            if i < self.S:
                p, dmg = self._reduction_bwd(i, st, dxin, grads, ready)
            dx = None
            if d_maps[i] is not None:
                dc = d_maps[i].to(self.dev, torch.float32).permute(0, 2, 3, 1).contiguous().view(n, C)
                dx = self._lnr_bwd(dc, st["out"], "norm%d." % i, grads)
            ready(self.group_end["norm%d" % i])
            if dmg is not None:
                acc = dx is not None
                if not acc:
                    dx = E(n, C)
                nb = hip.patch_merge_ln_bwd_nblocks(B, h, wd)
                part, gb = E(nb, 8 * C), E(8 * C)
                hip.patch_merge_ln_bwd(dmg, st["out"], w[p + "norm.weight"], dx, part, B, h, wd, C,
                                       self.EPS, accumulate=acc)
                hip.colsum(part, gb)
                grads[p + "norm.weight"].copy_(self._unfold_order(gb[:4 * C], C))
                grads[p + "norm.bias"].copy_(self._unfold_order(gb[4 * C:], C))
                ready(self.group_end[p + "norm"])
            if dx is None:
                raise ValueError("no gradient reaches stage %d: d_c%d is required" % (i, i + 2))
            for j in reversed(range(bb.depths[i])):
                q = "stages.%d.blocks.%d." % (i, j)
                dx = self._block_bwd(q, st["blocks"][j], dx, grads, B, h, wd, C, nh,
                                     None if keep is None else keep[st["blk0"] + j])
                ready(self.group_end[q[:-1]])
            dxin = dx
        if self.train_embed:
            self._patch_embed_bwd(dxin, grads)
            ready(self.group_end["patch_embed"])
        ready(self.flat_numel)
        return grads
