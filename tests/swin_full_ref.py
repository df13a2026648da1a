"""float64 statements of the two operators a fully trainable Swin backbone adds to the last-stage
tape -- the backward of patch merging's fused 2x2 gather + LayerNorm(4C) and the backward of the
4x4 patch embedding -- and a float32 / float64 autograd run through oracle/swin.py's own modules
over all stages (DropPath factors and mmdet's `_freeze_stages` included).  Shared by
tests/test_swin_full_refs.py (host: the statements against autograd) and tests/test_swin_full_gpu.py
(GPU: the kernels and the tape against the statements).  Not a test module."""
import copy

import torch
import torch.nn.functional as F

DIMS = dict(embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), window_size=4)
BATCH, IMG_H, IMG_W = 2, 50, 70          # maps 13x18, 7x9, 4x5, 2x3: every padding branch


def frozen(name, frozen_stages):
    """mmdet SwinTransformer._freeze_stages, restated (as tests/test_swin_grad_layout.py::_frozen):
    any frozen_stages >= 0 fixes patch_embed; stages[i - 1] and norm{i - 1} for 1 <= i <= frozen_stages."""
    if frozen_stages >= 0 and name.startswith("patch_embed."):
        return True
    for i in range(1, frozen_stages + 1):
        if name.startswith("stages.%d." % (i - 1)) or name.startswith("norm%d." % (i - 1)):
            return True
    return False


# ---------------------------------------------------------------- column orders of the 4C axis
def to_neighbour_major(t, C):
    """nn.Unfold order (c * 4 + row * 2 + col, the reference parameter's) -> (row * 2 + col) * C + c."""
    return t.reshape(*t.shape[:-1], C, 4).transpose(-1, -2).reshape(t.shape)


def to_unfold(t, C):
    return t.reshape(*t.shape[:-1], 4, C).transpose(-1, -2).reshape(t.shape)


# ---------------------------------------------------------------- patch merging + LayerNorm
def merge_gather(x, B, H, W, C):
    """x [B, H, W, C] -> the merged rows [B * H2 * W2, 4C], neighbour-major, zeros beyond an odd
    map's edge (the reference pads before nn.Unfold)."""
    xp = F.pad(x.reshape(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    H2, W2 = xp.shape[1] // 2, xp.shape[2] // 2
    return xp.view(B, H2, 2, W2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * H2 * W2, 4 * C)


def patch_merge_ln_bwd(dy, x, gamma, eps, B, H, W, C):
    """dy [rows, 4C] (d of the gathered, normalised rows), x [B, H, W, C], gamma [4C]
    neighbour-major -> (dx [B, H, W, C], d gamma [4C], d beta [4C]), float64.  The padding
    positions count in the row's moments and in both backward means; their dx is dropped."""
    dy, x, gamma = dy.double(), x.double(), gamma.double()
    g = merge_gather(x, B, H, W, C)
    mean = g.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((g - mean) ** 2).mean(1, keepdim=True) + eps)
    xhat = (g - mean) * rstd
    gd = dy * gamma
    dg = rstd * (gd - gd.mean(1, keepdim=True) - xhat * (gd * xhat).mean(1, keepdim=True))
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    dxp = dg.view(B, H2, W2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H2, 2 * W2, C)
    return dxp[:, :H, :W].contiguous(), (dy * xhat).sum(0), dy.sum(0)


# ---------------------------------------------------------------- patch embedding
def layernorm_bwd(dy, x, gamma, eps):
    dy, x, gamma = dy.double(), x.double(), gamma.double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (x - mean) * rstd
    gd = dy * gamma
    dx = rstd * (gd - gd.mean(-1, keepdim=True) - xhat * (gd * xhat).mean(-1, keepdim=True))
    return dx, (dy * xhat).reshape(-1, x.shape[-1]).sum(0), dy.reshape(-1, x.shape[-1]).sum(0)


def patch_cols(img):
    """img [B, 3, H, W] -> [B * h * w, 48] rows in the order c * 16 + ky * 4 + kx of a [C, 3, 4, 4]
    convolution weight; the image zero-padded bottom / right to multiples of 4."""
    B, _, H, W = img.shape
    p = F.pad(img.double(), (0, (4 - W % 4) % 4, 0, (4 - H % 4) % 4))
    h, w = p.shape[2] // 4, p.shape[3] // 4
    return p.view(B, 3, h, 4, w, 4).permute(0, 2, 4, 1, 3, 5).reshape(B * h * w, 48)


def patch_embed_bwd(img, d_out, weight, bias, gamma, eps):
    """Backward of PatchEmbed (Conv2d k = s = 4, then LayerNorm) for d_out [B * h * w, C], the
    gradient of its output tokens -> dict of the four parameter gradients, float64."""
    cols = patch_cols(img)
    C = weight.shape[0]
    proj = cols @ weight.double().reshape(C, 48).t() + bias.double()
    dproj, dgamma, dbeta = layernorm_bwd(d_out, proj, gamma, eps)
    return {"projection.weight": (dproj.t() @ cols).view(C, 3, 4, 4), "projection.bias": dproj.sum(0),
            "norm.weight": dgamma, "norm.bias": dbeta}


# ---------------------------------------------------------------- the whole backbone by autograd
def oracle_backward(oracle, img, d_maps, frozen_stages, keep=None, dtype=torch.float64):
    """Autograd through a copy of `oracle` (an oracle.swin.OracleSwin) in `dtype`: loss = sum over
    the output stages of (norm{i}(x_i) * d_maps[i]).sum(), d_maps[i] [B, h, w, C] or None.
    `keep` [sum(depths), 2, B]: DropPath factors; frozen stages ignore them (eval mode).
    Returns (maps [B, h, w, C] per stage, {state-dict name: gradient} of the trainable
    parameters the loss reaches -- a parameter without a gradient has no entry)."""
    m = copy.deepcopy(oracle).to(dtype)
    for n, p in m.named_parameters():
        p.requires_grad_(not frozen(n, frozen_stages))
    B = img.shape[0]
    x, hw = m.patch_embed(img.to(dtype))
    outs, loss, blk = [], 0.0, 0
    for i, st in enumerate(m.stages):
        for b in st.blocks:
            use = keep is not None and i >= max(frozen_stages, 0)
            sa = keep[blk, 0].to(dtype).view(B, 1, 1) if use else 1.0
            sf = keep[blk, 1].to(dtype).view(B, 1, 1) if use else 1.0
            x = x + sa * b.attn(b.norm1(x), hw)
            x = x + sf * b.ffn(b.norm2(x))
            blk += 1
        y = getattr(m, "norm%d" % i)(x).view(B, hw[0], hw[1], -1)
        outs.append(y.detach())
        if d_maps[i] is not None:
            loss = loss + (y * d_maps[i].to(dtype)).sum()
        if st.downsample is not None:
            x, hw = st.downsample(x, hw)
    loss.backward()
    return outs, {n: p.grad.detach() for n, p in m.named_parameters() if p.grad is not None}
