"""float64 statements behind the backward of the pixel decoder's FPN branch
(pair-net_amd/seg_grad.py `SegPixelDecoderGrad`, csrc/fpn_grad.hip):

  * the adjoint of the bilinear upsampling, as the transpose of the dense per-axis tap matrices
    built from `fwd_ref.taps`,
  * GroupNorm (+ gate) backward from the layer's input,
  * the branch itself (lateral 1x1 + GroupNorm, + upsampled finest memory, 3x3 + GroupNorm + ReLU,
    `mask_feature`) as autograd-able torch, with an optional externally supplied ReLU gate.

Each kernel statement returns the value and `mag`, the same computation on absolute values, as
tests/fwd_ref.py does.  tests/test_fpn_grad_refs.py pins them to torch / the oracle;
tests/test_fpn_grad_kernels_gpu.py and tests/test_fpn_grad_gpu.py bound the GPU against them."""
import torch
import torch.nn.functional as F

import fwd_ref as R

U = R.U
ADJ_COORD = 3        # src = scale (dst + 0.5) - 0.5: the quotient, the product, the difference
PD = "pixel_decoder."
BRANCH_PARAMS = [PD + n for n in (
    "mask_feature.weight", "mask_feature.bias", "output_convs.0.conv.weight",
    "output_convs.0.gn.weight", "output_convs.0.gn.bias", "lateral_convs.0.conv.weight",
    "lateral_convs.0.gn.weight", "lateral_convs.0.gn.bias")]


# ------------------------------------------------------------------------------ bilinear adjoint
def tap_matrix(n_in, n_out, device="cpu"):
    """T [n_out][n_in] float64 with out = T in along one axis: row o holds l0 at i0 and l1 at i1
    (both on one column at the clamped last index: added)."""
    i0, i1, l0, l1, _ = R.taps(n_in, n_out, device)
    T = torch.zeros(n_out, n_in, dtype=torch.float64, device=device)
    o = torch.arange(n_out, device=device)
    T.index_put_((o, i0), l0, accumulate=True)
    T.index_put_((o, i1), l1, accumulate=True)
    return T


def window(i, n_in, n_out):
    """The fine indices that can tap coarse index i: src = in / out (dst + 0.5) - 0.5 within
    (i - 1, i + 1), inverted in integers and widened by one on each side, clipped to the axis."""
    a, b = (2 * i - 1) * n_out - n_in, (2 * i + 3) * n_out - n_in
    # integers inside the open interval are floor(lo) + 1 .. ceil(hi) - 1: one more on each side
    lo = a // (2 * n_in)                           # (Python's // floors)
    hi = -((-b) // (2 * n_in))
    return max(lo, 0), min(hi, n_out - 1)


def window_matrix(n_in, n_out, device="cpu"):
    W = torch.zeros(n_out, n_in, dtype=torch.float64, device=device)
    for i in range(n_in):
        lo, hi = window(i, n_in, n_out)
        W[lo:hi + 1, i] = 1.0
    return W


def bilinear_adjoint(g, hi, wi):
    """g [..., ho, wo] -> (d [..., hi, wi], mag, extra): d = Ty^T g Tx.  extra (in units of 2^-24):
    a fine row's (column's) coordinate off by f of a pixel moves its two weights by f, hence d by
    at most f sum |g| over the candidate window; f = ADJ_COORD (1 + in) 2^-24 per axis."""
    ho, wo = g.shape[-2:]
    g64 = g.double()
    Ty, Tx = tap_matrix(hi, ho, g.device), tap_matrix(wi, wo, g.device)
    d = torch.einsum("oi,...op,pj->...ij", Ty, g64, Tx)
    mag = torch.einsum("oi,...op,pj->...ij", Ty, g64.abs(), Tx)
    Wy, Wx = window_matrix(hi, ho, g.device), window_matrix(wi, wo, g.device)
    win = torch.einsum("oi,...op,pj->...ij", Wy, g64.abs(), Wx)
    return d, mag, ADJ_COORD * (2.0 + hi + wi) * win


def adjoint_contributors(n_in, n_out):
    """The largest number of fine indices inside one coarse index's candidate window."""
    return max(hi - lo + 1 for lo, hi in (window(i, n_in, n_out) for i in range(n_in)))


# ------------------------------------------------------------------------------ GroupNorm backward
def group_norm_bwd(x, dy, gamma, G, eps, gate=None, dtype=torch.float64):
    """x, dy [B][HW][C] (the layer's INPUT and the gradient of its output), gate [B][HW][C] of
    0 / 1 or None -> dict(dx, dgamma, dbeta, and the `_mag` of each, cnt_stats):
        g = gamma dy gate, xhat = (x - mean) rstd, m1 = mean g, m2 = mean(g xhat) per (image, group)
        dx = rstd (g - m1 - xhat m2),  dgamma = sum dy gate xhat,  dbeta = sum dy gate.
    mags: the same on absolute values with xhat -> (|x| + |mean|) rstd (the TRUE rstd, as
    fwd_ref.layer_norm argues).  cnt_stats: the statistics come from double sums, whose relative
    error n 2^-53 on E[x^2] + mean^2 moves rstd by n 2^-53 (E[x^2] + mean^2) / (2 (var + eps));
    dx carries rstd twice, dgamma once: that many 2^-24 of mag (fwd_ref.group_norm_nhwc)."""
    B, HW, C = x.shape
    cpg = C // G
    n = HW * cpg
    sh = (B, HW, G, cpg)
    x_, d_ = x.to(dtype).reshape(sh), dy.to(dtype).reshape(sh)
    if gate is not None:
        d_ = d_ * gate.to(dtype).reshape(sh)
    gam = gamma.to(dtype).reshape(1, 1, G, cpg)
    mean = x_.mean((1, 3), keepdim=True)
    var = ((x_ - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x_ - mean) * rstd
    g = gam * d_
    m1, m2 = g.mean((1, 3), keepdim=True), (g * xh).mean((1, 3), keepdim=True)
    out = dict(dx=(rstd * (g - m1 - xh * m2)).reshape(B, HW, C),
               dgamma=(d_ * xh).sum((0, 1)).reshape(C), dbeta=d_.sum((0, 1)).reshape(C))
    xhm = (x_.abs() + mean.abs()) * rstd
    ga = g.abs()
    m1m, m2m = ga.mean((1, 3), keepdim=True), (ga * xhm).mean((1, 3), keepdim=True)
    out["dx_mag"] = (rstd * (ga + m1m + xhm * m2m)).reshape(B, HW, C)
    out["dgamma_mag"] = (d_.abs() * xhm).sum((0, 1)).reshape(C)
    out["dbeta_mag"] = d_.abs().sum((0, 1)).reshape(C)
    ex2 = (x_ * x_).mean((1, 3), keepdim=True)
    rel = n * 2.0 ** -53 * (ex2 + mean * mean) / (2.0 * (var + eps)) / U
    out["cnt_stats"] = float(rel.max())
    return out


# ------------------------------------------------------------------------------ the branch
def branch_params(pixel_decoder):
    """The eight tensors of the branch from an oracle MSDeformAttnPixelDecoder, by reference name."""
    sd = dict(pixel_decoder.named_parameters())
    return {PD + k: sd[k] for k in (n[len(PD):] for n in BRANCH_PARAMS)}


def branch(c2, mem2, p, G, gate=None, eps=1e-5):
    """c2 [B, C, H2, W2], mem2 [B, 256, h2, w2] (the finest memory level as a map), p: reference
    parameter name -> tensor -> (MF [B, 256, H2, W2], z: the 3x3's GroupNorm output BEFORE the
    ReLU).  `gate` ([B, 256, H2, W2] of 0 / 1): out = z gate instead of relu(z) -- the same value
    wherever gate = (z > 0), and the gate's own derivative everywhere."""
    cur = F.group_norm(F.conv2d(c2, p[PD + "lateral_convs.0.conv.weight"]), G,
                       p[PD + "lateral_convs.0.gn.weight"], p[PD + "lateral_convs.0.gn.bias"], eps)
    y = cur + F.interpolate(mem2, size=cur.shape[-2:], mode="bilinear", align_corners=False)
    z = F.group_norm(F.conv2d(y, p[PD + "output_convs.0.conv.weight"], padding=1), G,
                     p[PD + "output_convs.0.gn.weight"], p[PD + "output_convs.0.gn.bias"], eps)
    out = F.relu(z) if gate is None else z * gate.to(z.dtype)
    return F.conv2d(out, p[PD + "mask_feature.weight"], p[PD + "mask_feature.bias"]), z


def gate_mismatch(gate, z64):
    """Fraction of elements where a 0 / 1 gate differs from the float64 statement's own sign."""
    return float(((gate > 0) != (z64 > 0)).double().mean())


GATE_CAP = 1e-3
