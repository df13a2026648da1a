"""float64 statements of the forward kernels every inference step and every taped forward run
through: the softmax attentions (csrc/attn.hip, csrc/swin.hip), the normalisations (csrc/norm.hip,
k_ln_rows of csrc/swin.hip), the deformable and bilinear samplers (csrc/msda.hip, csrc/resize.hip),
the fused FFN (csrc/ffn.hip) and the exact GELU, written from the formulas in the kernels'
headers.  Each returns the value and `mag`, the same computation on absolute values (subtractions
become additions), and -- where an exponential, a reciprocal square root or a sampling coordinate
sits between input and output -- the conditioning terms a bound needs, computed from the inputs
alone.  tests/test_fwd_refs.py pins every statement to the torch / oracle function it restates
(1e-12); tests/test_fwd_kernels_gpu.py bounds the kernels against them.  Inputs are fp32 tensors
(any device); all arithmetic is float64; loops where a loop is the clearest statement."""
import math

import torch

U = 2.0 ** -24
LOG2E = 1.4426950408889634
Z_MAX = 88.0      # exp(-88) < FLT_MIN: entries further below their row's largest are covered by
                  # the additive FLT_MIN of the bound (labnotes/r14.md, `z`)
SCORE_CHAIN = 34  # q * (scale log2 e): 2 roundings; 16 MFMAs of two products each: 32


# ------------------------------------------------------------------------------ normalisations
def layer_norm(x, gamma, beta, eps, xmag=None):
    """LayerNorm over the last dim -> (y, mag, amp, amp2).
    d = x - mean(x), y = d rstd gamma + beta with rstd = (mean(d^2) + eps)^-1/2.
    mag = (xmag + mean(xmag)) rstd |gamma| + |beta|, xmag = |x| unless the caller's rows carry
    a magnitude of their own: the subtraction on absolute values, times the TRUE rstd (a sum of
    squares has no signs to drop; 1 / sqrt of the absolute moments would understate a row
    whose mean dwarfs its spread).
    The conditioning of rstd: perturbing d_j by |e_j| <= L 2^-24 dm_j (dm = xmag + mean xmag)
    moves var by 2 mean(d e) + mean(e^2), hence rstd by at most
        L 2^-24 mean(|d| dm) / (var + eps)  +  (L 2^-24)^2 mean(dm^2) / (2 (var + eps))
    relative.  Per element, as a multiple of 2^-24 mag:
        amp  = |d rstd gamma| / mag * mean(|d| dm) / (var + eps)          (times L)
        amp2 = |d rstd gamma| / mag * 2^-24 mean(dm^2) / (2 (var + eps))  (times L^2)"""
    x64, g, b = x.double(), gamma.double(), beta.double()
    mean = x64.mean(-1, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd * g + b
    xm = x64.abs() if xmag is None else xmag.double()
    dm = xm + xm.mean(-1, keepdim=True)
    mag = dm * rstd * g.abs() + b.abs()
    share = (d * rstd * g).abs() / mag.clamp_min(1e-300)
    amp = share * (d.abs() * dm).mean(-1, keepdim=True) / (var + eps)
    amp2 = share * U * (dm * dm).mean(-1, keepdim=True) / (2.0 * (var + eps))
    return y, mag, amp, amp2


def group_norm_nhwc(x, gamma, beta, G, eps, relu):
    """GroupNorm of channel-last x [B][HW][C] over (HW, C / G) -> (y, mag, cnt_stats).
    mag as layer_norm's.  cnt_stats: the kernel forms var = E[x^2] - mean^2 from DOUBLE sums;
    their relative error n 2^-53 on E[x^2] + mean^2 moves rstd by n 2^-53 (E[x^2] + mean^2) /
    (2 (var + eps)), which on the element is that many 2^-24 mag:
        cnt_stats = |d rstd gamma| / mag * n 2^-53 (E[x^2] + mean^2) / (2 (var + eps) 2^-24).
    ReLU is 1-Lipschitz: max(y, 0) inherits y's bound with y's mag."""
    B, HW, C = x.shape
    x64 = x.double().reshape(B, HW, G, C // G)
    n = HW * (C // G)
    mean = x64.mean((1, 3), keepdim=True)
    d = x64 - mean
    var = (d * d).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    g = gamma.double().reshape(1, 1, G, C // G)
    b = beta.double().reshape(1, 1, G, C // G)
    y = d * rstd * g + b
    dm = x64.abs() + x64.abs().mean((1, 3), keepdim=True)
    mag = dm * rstd * g.abs() + b.abs()
    ex2 = (x64 * x64).mean((1, 3), keepdim=True)
    rel = n * 2.0 ** -53 * (ex2 + mean * mean) / (2.0 * (var + eps))
    cnt = (d * rstd * g).abs() / mag.clamp_min(1e-300) * rel / U
    if relu:
        y = y.clamp_min(0.0)
    return y.reshape(B, HW, C), mag.reshape(B, HW, C), cnt.reshape(B, HW, C)


def l2_normalize(x, eps):
    """x / max(||x||, eps) over the last dim -> (y, mag); nothing is subtracted: mag = |y|."""
    x64 = x.double()
    n = torch.sqrt((x64 * x64).sum(-1, keepdim=True))
    y = x64 / n.clamp_min(eps)
    return y, y.abs()


def gelu(x):
    """x Phi(x) = 0.5 x (1 + erf(x / sqrt 2)) -> (y, mag = 0.5 |x| (1 + |erf|)): for x << 0 the
    sum 1 + erf cancels, which mag keeps."""
    x64 = x.double()
    e = torch.erf(x64 / math.sqrt(2.0))
    return 0.5 * x64 * (1.0 + e), 0.5 * x64.abs() * (1.0 + e.abs())


# ------------------------------------------------------------------------------ bilinear resize
def taps(n_in, n_out, device="cpu"):
    """ATen's upsample_bilinear2d source index, align_corners=False, no scale factor:
    src = max(in / out (dst + 0.5) - 0.5, 0); i0 = min(floor(src), in - 1);
    i1 = i0 + (i0 < in - 1); l1 = src - i0; l0 = 1 - l1 -> (i0, i1, l0, l1, src)."""
    dst = torch.arange(n_out, dtype=torch.float64, device=device)
    src = ((float(n_in) / float(n_out)) * (dst + 0.5) - 0.5).clamp_min(0.0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = src - i0.double()
    return i0, i1, 1.0 - l1, l1, src


def bilinear(x, ho, wo):
    """x [..., hi, wi] -> (y [..., ho, wo], mag, spread): y = l0y (l0x v00 + l1x v01) +
    l1y (l0x v10 + l1x v11); spread = the largest difference between two of the four taps, by
    which a coordinate that is off by a fraction f of a pixel (either axis) moves the sample:
    |dy| <= f spread per axis."""
    hi, wi = x.shape[-2:]
    x64 = x.double()
    y0, y1, ly0, ly1, _ = taps(hi, ho, x.device)
    x0, x1, lx0, lx1, _ = taps(wi, wo, x.device)
    v00, v01 = x64[..., y0, :][..., x0], x64[..., y0, :][..., x1]
    v10, v11 = x64[..., y1, :][..., x0], x64[..., y1, :][..., x1]
    ly0, ly1 = ly0[:, None], ly1[:, None]
    y = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
    mag = ly0 * (lx0 * v00.abs() + lx1 * v01.abs()) + ly1 * (lx0 * v10.abs() + lx1 * v11.abs())
    four = torch.stack([v00, v01, v10, v11])
    return y, mag, four.amax(0) - four.amin(0)


def stencil_index(hi, wi, ho, wo, nudge=0.0):
    """Source pixel (row-major index into hi x wi) of tap t = 2 (row tap) + (column tap) of
    every output pixel, tap-major [4][ho * wo], as pn_bilinear_stencil_rows_f32 orders its
    rows.  `nudge` moves every source coordinate by that many pixels before the floor: a
    coordinate within rounding of an integer may fall either side of it in fp32."""
    def axis(n_in, n_out):
        dst = torch.arange(n_out, dtype=torch.float64)
        src = ((float(n_in) / float(n_out)) * (dst + 0.5) - 0.5 + nudge).clamp_min(0.0)
        i0 = src.floor().long().clamp_max(n_in - 1)
        return i0, i0 + (i0 < n_in - 1).long()
    ys, xs = axis(hi, ho), axis(wi, wo)
    return torch.stack([(ys[t >> 1][:, None] * wi + xs[t & 1][None, :]).reshape(-1)
                        for t in range(4)])


# ------------------------------------------------------------------------------ deformable sampling
def msda(value, shapes, loc, aw, z=None):
    """mmcv's multi_scale_deformable_attn: value [B][N][8][32], N = sum h w level-major;
    loc [B][Nq][8][L][4][2] as (x, y) in [0, 1]; aw [B][Nq][8][L][4] ->
    (out [B][Nq][256], mag, spread, ix, iy, cnt).
    Per level: pixel coordinates ix = x w - 0.5, iy = y h - 0.5 (grid_sample,
    align_corners=False); the four taps around (ix, iy) with bilinear weights; a tap outside the
    map contributes ZERO (zero padding, not the clamped border pixel).
      out    = sum_{l,p} aw * sum_taps wt * v
      mag    = sum_{l,p} |aw| * sum_taps wt * |v|
      spread = sum_{l,p} |aw| * (max - min over the four zero-padded taps) * reach, with
      reach  = 1 + |ix| + |iy| + max(h, w): a coordinate carried through k fp32 roundings is off
               by at most k 2^-24 reach of a pixel and moves the sample by that times the taps'
               largest difference.
      cnt    = with z [B][Nq][8][L][4] the roundings each weight inherits through its exponent
               (msda_encoder_inputs): sum aw z |sample| / mag + sum aw z per head, as
               softmax_av's cnt_exp; zero without z."""
    B, N, NH, D = value.shape
    Nq, L = loc.shape[1], loc.shape[3]
    v64, loc64, aw64 = value.double(), loc.double(), aw.double()
    out = torch.zeros(B, Nq, NH, D, dtype=torch.float64, device=value.device)
    mag, spread, zmag = torch.zeros_like(out), torch.zeros_like(out), torch.zeros_like(out)
    zsum = torch.zeros(B, Nq, NH, 1, dtype=torch.float64, device=value.device)
    bi = torch.arange(B, device=value.device).view(B, 1, 1, 1)
    hd = torch.arange(NH, device=value.device).view(1, 1, NH, 1)
    start, ixs, iys = 0, [], []
    for l, (h, w) in enumerate(shapes):
        ix = loc64[:, :, :, l, :, 0] * w - 0.5            # [B][Nq][8][4]
        iy = loc64[:, :, :, l, :, 1] * h - 0.5
        x0, y0 = ix.floor(), iy.floor()
        tx, ty = ix - x0, iy - y0
        tapv = []
        s, m = 0.0, 0.0
        for dy, dx, wt in ((0, 0, (1 - tx) * (1 - ty)), (0, 1, tx * (1 - ty)),
                           (1, 0, (1 - tx) * ty), (1, 1, tx * ty)):
            xx, yy = x0 + dx, y0 + dy
            inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            idx = start + yy.clamp(0, h - 1).long() * w + xx.clamp(0, w - 1).long()
            tv = v64[bi, idx, hd] * inside[..., None]      # [B][Nq][8][4][32]
            tapv.append(tv)
            s = s + wt[..., None] * tv
            m = m + wt[..., None] * tv.abs()
        four = torch.stack(tapv)
        reach = 1.0 + ix.abs() + iy.abs() + float(max(h, w))
        a = aw64[:, :, :, l, :, None]
        out += (a * s).sum(3)
        mag += (a.abs() * m).sum(3)
        spread += (a.abs() * (four.amax(0) - four.amin(0)) * reach[..., None]).sum(3)
        if z is not None:
            az = a.abs() * z.double()[:, :, :, l, :, None]
            zmag += (az * m).sum(3)
            zsum += az.sum(3)
        ixs.append(ix)
        iys.append(iy)
        start += h * w
    cnt = zmag / mag.clamp_min(1e-300) + zsum
    flat = lambda t: t.reshape(B, Nq, NH * D)
    return flat(out), flat(mag), flat(spread), torch.stack(ixs, 3), torch.stack(iys, 3), flat(cnt)


def msda_encoder_inputs(offsets, logits, shapes):
    """The encoder entry's inputs (pn_msda_f32) as the operator's: every token of every level is
    a query at its own pixel centre, reference point ((qx + 0.5) / qw, (qy + 0.5) / qh) at
    EVERY level; loc = ref + offset / (w_l, h_l); aw = softmax over the head's L * 4 logits.
    offsets [B][N][8][L][4][2], logits [B][N][8][L*4] -> (loc, aw, z) with z = max logit -
    logit (<= 88): the roundings the weight inherits through its exponent."""
    B, N, NH, L = offsets.shape[:4]
    dev = offsets.device
    ref = []
    for h, w in shapes:
        for qy in range(h):
            for qx in range(w):
                ref.append(((qx + 0.5) / w, (qy + 0.5) / h))
    ref = torch.tensor(ref, dtype=torch.float64, device=dev)                 # [N][2]
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64, device=dev)
    loc = ref[None, :, None, None, None, :] + offsets.double() / norm[None, None, None, :, None, :]
    lg = logits.double()
    z = (lg.amax(-1, keepdim=True) - lg).clamp_max(Z_MAX)
    aw = torch.softmax(lg, -1)
    return loc, aw.view(B, N, NH, L, 4), z.view(B, N, NH, L, 4)


# ------------------------------------------------------------------------------ softmax attention
def softmax_av(s, E, v):
    """Rows of scores s [..., Nq, Nk] (natural units, -inf = masked; at least one live key per
    row), E the bound on each score's own rounding error in units of 2^-24 (from the inputs),
    values v [..., Nk, D] -> (out, mag, cnt_exp, cnt_score), all [..., Nq, D] but cnt_score
    [..., Nq, 1].
      p = softmax(s); out = p v; mag = p |v|.
      cnt_exp: s - m is rounded once per exponential it passes (the online softmax re-bases a
        numerator from one running maximum to the next: the differences telescope to M - s_j),
        and the exponential turns that absolute error into a relative one: p_j carries
        z_j = min(88, M - s_j) roundings.  A relative error z_j on p_j moves the quotient
        sum p v / sum p by at most sum_j p_j z_j |v_j| + mag sum_j p_j z_j:
            cnt_exp = (p z) |v| / mag + sum_j p_j z_j.
      cnt_score: the score of key j is off by at most E_j 2^-24 (times log2 e in the kernel's
        log2 units); to first order p_j moves by twice the largest such error over the row's
        keys that contribute, relative: cnt_score = 2 log2(e) max_j E_j over the keys with
        z_j < 88 (a key further below the maximum, such as one behind the -100 of a window's
        region mask, weighs less than FLT_MIN and grants nothing)."""
    live = torch.isfinite(s)
    M = s.amax(-1, keepdim=True)
    e = torch.exp(s - M)
    p = e / e.sum(-1, keepdim=True)
    va = v.abs()
    out, mag = p @ v, p @ va
    z = torch.where(live, (M - s).clamp_max(Z_MAX), torch.zeros_like(s))
    pz = p * z
    cnt_exp = (pz @ va) / mag.clamp_min(1e-300) + pz.sum(-1, keepdim=True)
    counts = live & ((M - s) < Z_MAX)
    cnt_score = 2.0 * LOG2E * torch.where(counts, E, torch.zeros_like(E)).amax(-1, keepdim=True)
    return out, mag, cnt_exp, cnt_score


def attention(q, k, v, mask, scale):
    """8 heads x 32: q [B][Q][256], k / v [B][Nk][256], mask [B][Q][Nk] bool (True = the key is
    masked) or None.  A row whose keys are ALL masked attends to every key (`rowall` un-masks it:
    Mask2Former's attn_mask[attn_mask.sum(-1) == Nk] = False) -> softmax_av's four, [B][Q][256]
    (cnt_score [B][Q][8] repeated over the head's 32 channels)."""
    B, Q, _ = q.shape
    Nk = k.shape[1]
    qh = q.double().view(B, Q, 8, 32).transpose(1, 2)
    kh = k.double().reshape(B, Nk, 8, 32).transpose(1, 2)
    vh = v.double().reshape(B, Nk, 8, 32).transpose(1, 2)
    s = scale * (qh @ kh.transpose(-1, -2))
    # SCORE_CHAIN roundings on scale sum_d |q_d k_jd|
    E = SCORE_CHAIN * abs(scale) * (qh.abs() @ kh.abs().transpose(-1, -2))
    if mask is not None:
        m = mask.clone()
        m[m.all(-1)] = False
        s = s.masked_fill(m[:, None], float("-inf"))
    out, mag, ce, cs = softmax_av(s, E, vh)
    back = lambda t: t.transpose(1, 2).reshape(B, Q, 256)
    return back(out), back(mag), back(ce), back(cs.expand(-1, -1, -1, 32))


def window_attention(qkv, qkv_bias, table, B, H, W, C, heads, ws, shift, scale):
    """(Shifted-)window attention of Swin on qkv rows [B*H*W][3C] (q | k | v, head-major 32s);
    table [heads][(2 ws - 1)^2] -> softmax_av's four as [B*H*W][C].
    The map is padded on the bottom / right to multiples of ws and rolled by -shift.  A PADDED
    token's q / k / v row IS `qkv_bias` (the reference pads after norm1 with zeros, so its qkv
    projection is the bias alone); it is a key like any other, and its own output is dropped.
    Score of query t, key u of a window: scale q_t . k_u + table[head][(ty - uy + ws - 1)
    (2 ws - 1) + (tx - ux + ws - 1)], and -100 where shift > 0 and the two tokens come from
    different wrap-around regions (rows / columns >= Hp - ws and >= Hp - shift of the rolled map
    each start a new one).  Rounding of a score, in units of 2^-24: SCORE_CHAIN on the q . k
    magnitude; the bias entry times log2 e and its addition: |bias| + (|q . k| + |bias|); the
    region term's addition: the whole magnitude once more."""
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    dev = qkv.device
    rows = torch.cat([qkv.double()[:, :3 * C], qkv_bias.double()[None, :3 * C]])   # last = padding
    pad = rows.shape[0] - 1
    tab = table.double()
    N = ws * ws
    py, px = torch.arange(N, device=dev) // ws, torch.arange(N, device=dev) % ws
    rel = (py[:, None] - py[None, :] + ws - 1) * (2 * ws - 1) + (px[:, None] - px[None, :] + ws - 1)
    outs = [torch.zeros(B * H * W, C, dtype=torch.float64, device=dev) for _ in range(3)]
    score = torch.zeros(B * H * W, C, dtype=torch.float64, device=dev)
    region = lambda c, n: (c >= n - ws).long() + (c >= n - shift).long()
    for b in range(B):
        for wy in range(Hp // ws):
            for wx in range(Wp // ws):
                y, x = wy * ws + py, wx * ws + px                 # in the padded, rolled map
                ys, xs = (y + shift) % Hp, (x + shift) % Wp       # source pixel
                real = (ys < H) & (xs < W)
                src = torch.where(real, (b * H + ys) * W + xs, torch.full_like(ys, pad))
                label = region(y, Hp) * 3 + region(x, Wp) if shift > 0 else torch.zeros_like(y)
                far = label[:, None] != label[None, :]
                t = rows[src].view(N, 3, heads, 32).permute(1, 2, 0, 3)     # [3][heads][N][32]
                s = scale * (t[0] @ t[1].transpose(-1, -2)) + tab[:, rel]
                S = abs(scale) * (t[0].abs() @ t[1].abs().transpose(-1, -2))
                ba = tab[:, rel].abs()
                s = s - 100.0 * far
                E = SCORE_CHAIN * S + ba + (S + ba) + (S + ba + 100.0 * far)
                res = softmax_av(s, E, t[2])
                dst = src[real]
                for o, r in zip(outs, res[:3]):
                    o[dst] = r.permute(1, 0, 2).reshape(N, C)[real]
                score[dst] = res[3].expand(-1, -1, 32).permute(1, 0, 2).reshape(N, C)[real]
    return outs[0], outs[1], outs[2], score


# ------------------------------------------------------------------------------ patch merging, FFN
def patch_merge_gather(x, B, H, W, C):
    """x [B][H*W][C] -> [B][ceil(H/2) ceil(W/2)][4C]: the 2 x 2 neighbourhood of (2 y2, 2 x2)
    concatenated neighbour-major, column (dy * 2 + dx) * C + c <- pixel (2 y2 + dy, 2 x2 + dx);
    a neighbour outside an odd map is ZERO and enters the row's statistics as zeros."""
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    x64 = x.double().view(B, H, W, C)
    out = torch.zeros(B, H2, W2, 4 * C, dtype=torch.float64, device=x.device)
    for dy in range(2):
        for dx in range(2):
            q = dy * 2 + dx
            part = x64[:, dy::2, dx::2]
            out[:, :part.shape[1], :part.shape[2], q * C:(q + 1) * C] = part
    return out.view(B, H2 * W2, 4 * C)


def patch_merge_ln(x, gamma, beta, B, H, W, C, eps):
    """LayerNorm(4C) of patch_merge_gather's rows -> layer_norm's four."""
    return layer_norm(patch_merge_gather(x, B, H, W, C), gamma, beta, eps)


def ffn_pre(x, W1, b1, W2, b2):
    """u = x + relu(x W1^T + b1) W2^T + b2 -> (u, umag, h, hmag): hmag = |x| |W1|^T + |b1|;
    umag = |x| + hmag |W2|^T + |b2| -- ReLU is 1-Lipschitz, so the hidden row's error is
    bounded through hmag whichever side of zero it falls, and no element has to be left out."""
    x64, W1d, W2d = x.double(), W1.double(), W2.double()
    h = x64 @ W1d.T + b1.double()
    hmag = x64.abs() @ W1d.abs().T + b1.double().abs()
    u = x64 + h.clamp_min(0.0) @ W2d.T + b2.double()
    umag = x64.abs() + hmag @ W2d.abs().T + b2.double().abs()
    return u, umag, h, hmag
