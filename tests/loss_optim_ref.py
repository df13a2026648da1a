"""float64 statements of the loss-value, match-cost, point-sample and optimizer kernels
(csrc/loss.hip, csrc/optim.hip), written from the formulas in the kernels' headers.  Each returns
the value and, where a bound needs it, `mag`: the same computation on absolute values
(subtractions become additions).  tests/test_loss_optim_refs.py pins every statement to the
oracle / torch function it restates (1e-12); tests/test_loss_optim_kernels_gpu.py bounds the
kernels against them.  Inputs are fp32 tensors (any device); all arithmetic is float64."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def f32(x):
    """The fp32 rounding of a Python double, as a Python double."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------ mean losses
def ce_mean(x, t, cw, lw):
    """lw / n_kept sum_{t >= 0} cw[t] (logsumexp(x) - x[t]) -> (value, mag); (0, 0) without a
    kept row."""
    kept = t >= 0
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    if not bool(kept.any()):
        return zero, zero
    x64, y = x.double()[kept], t[kept]
    lse = torch.logsumexp(x64, -1)
    xy = x64.gather(1, y[:, None])[:, 0]
    w = torch.ones_like(lse) if cw is None else cw.double()[y]
    n = float(kept.sum())
    return lw / n * (w * (lse - xy)).sum(), lw / n * (w * (lse.abs() + xy.abs())).sum()


def seesaw_mean(x, t, cum, p, q, eps, lw):
    """mmdet SeesawLoss, class part, mean over the kept rows -> (value, mag).
    x'[j] = x[j] + log w[j] (j != y); per row mag = |logsumexp(x')| + |x[y]| + max_j (|x[j]| +
    |log w[j]|): the last term carries the roundings of the shifted logits into the logsumexp."""
    kept = t >= 0
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    if not bool(kept.any()):
        return zero, zero
    x64, y = x.double()[kept], t[kept]
    rows = torch.arange(x64.shape[0], device=x.device)
    w = torch.ones_like(x64)
    if p > 0:
        c = cum.double().clamp(min=1.0)
        ratio = c[None, :] / c[y][:, None]
        w = w * torch.where(ratio < 1.0, ratio.pow(p), torch.ones_like(ratio))
    if q > 0:
        s = torch.softmax(x64, -1)
        ratio = s / s[rows, y].clamp(min=eps)[:, None]
        w = w * torch.where(ratio > 1.0, ratio.pow(q), torch.ones_like(ratio))
    logw = w.log()
    logw[rows, y] = 0.0
    xs = x64 + logw
    lse, xy = torch.logsumexp(xs, -1), x64[rows, y]
    n = float(kept.sum())
    mag = lse.abs() + xy.abs() + (x64.abs() + logw.abs()).amax(-1)
    return lw / n * (lse - xy).sum(), lw / n * mag.sum()


def bce_posw_mean(x, t, lw):
    """BCEWithLogitsLoss(pos_weight = n / #(t > 0), mean) * lw -> (value, mag, pw as the fp32
    quotient of the two fp32 counts)."""
    x64, t64 = x.double().reshape(-1), t.double().reshape(-1)
    n = x64.numel()
    cnt = int((t64 > 0).sum())
    pw32 = np.float32(n) / np.float32(cnt)
    pw = float(n) / float(cnt)
    lwi = 1.0 + (pw - 1.0) * t64
    sp = F.softplus(-x64)
    val = lw / n * ((1.0 - t64) * x64 + lwi * sp).sum()
    mag = lw / n * (((1.0 - t64) * x64).abs() + lwi * sp).sum()
    return val, mag, pw32


# ------------------------------------------------------------------------------ match costs
def mask_match_cost(cls, labels, x, t, w_cls, w_mask, w_dice, eps):
    """MaskHungarianAssigner's cost [Q][G] -> (cost, mag); mag = the three terms' magnitudes."""
    c64, x64, t64 = cls.double(), x.double(), t.double()
    Np = x64.shape[1]
    c_cls = -torch.softmax(c64, -1)[:, labels] * w_cls
    neg = F.softplus(x64).sum(-1)[:, None]                      # sum_p BCE(x, 0)
    c_mask = (neg - x64 @ t64.T) / Np * w_mask
    m_mask = (neg + x64.abs() @ t64.abs().T) / Np * abs(w_mask)
    s = torch.sigmoid(x64)
    frac = (2.0 * (s @ t64.T) + eps) / (s.sum(-1)[:, None] + t64.sum(-1)[None, :] + eps)
    c_dice = (1.0 - frac) * w_dice
    m_dice = (1.0 + frac) * abs(w_dice)
    return (c_cls + c_mask) + c_dice, c_cls.abs() + m_mask + m_dice


def id_match_cost(sub, obj, rel, gs, go, gr, ws, wo, wr):
    """IdMatcher's cost [R][G] -> (cost, mag)."""
    a = torch.softmax(sub.double(), -1)[:, gs] * ws
    b = torch.softmax(obj.double(), -1)[:, go] * wo
    c = torch.softmax(rel.double(), -1)[:, gr] * wr
    return -a - b - c, a.abs() + b.abs() + c.abs()


def mask_cost_case(Q, G, Np, ncls, seed):
    """Inputs of one mask_match_cost case, drawn on the host (the CPU and the GPU tests see the
    same numbers): logits at scale 3 with planted +-80 entries and query Q - 1 at -80 everywhere;
    fractional targets in [0, 1], ground-truth row 0 all zeros and row G - 1 all ones (G >= 2);
    labels that include 0 and ncls - 2.  From G >= 3 and Q >= G, query g (g < G - 1; Q - 1 for the
    all-zero row 0) carries the logit of target g, so that it is by far that row's best match:
    the planted margin of the assignment cases."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(Q, ncls, generator=g) * 3.0
    x = torch.randn(Q, Np, generator=g) * 3.0
    t = torch.rand(G, Np, generator=g).round() * torch.rand(G, Np, generator=g)
    labels = torch.randint(0, ncls - 1, (G,), generator=g)
    labels[0] = 0
    labels[-1] = ncls - 2
    if G >= 2:
        t[0] = 0.0
        t[-1] = 1.0
    planted = {}
    if G >= 3 and Q >= G:
        for j in range(G):
            q = Q - 1 if j == 0 else j
            planted[q] = j
            if j > 0:
                x[q] = torch.logit(t[j].clamp(1e-4, 1.0 - 1e-4))
                cls[q, labels[j]] += 6.0
    x[0, ::5] = 80.0
    x[0, 1::5] = -80.0
    x[Q - 1] = -80.0
    cls[0, 0], cls[0, 1] = 80.0, -80.0
    return cls, labels, x, t, planted


def assignment_margin(cost, rows, cols):
    """For every assigned (row, col): the smallest other entry of the row minus the assigned
    one (float64 cost matrix; +inf with a single column)."""
    c = cost.detach().cpu().double().numpy()
    out = []
    for r, k in zip(rows, cols):
        rest = np.delete(c[r], k)
        out.append((rest.min() if rest.size else np.inf) - c[r, k])
    return np.asarray(out)


# ------------------------------------------------------------------------------ point sample
def point_grid(pts):
    """The fp32 grid coordinate 2 p - 1 the kernel starts from (one rounding, shared)."""
    return 2.0 * pts.float() - 1.0


def point_sample(maps, pts):
    """grid_sample(maps [P][h][w], 2 p - 1, bilinear, zeros, align_corners=False) -> (out [P][Np],
    largest |tap| of each map [P]); float64 from the fp32 grid coordinate."""
    P, h, w = maps.shape
    m = maps.double()
    c = point_grid(pts).double()
    ix, iy = ((c[:, 0] + 1.0) * w - 1.0) / 2.0, ((c[:, 1] + 1.0) * h - 1.0) / 2.0
    fx, fy = torch.floor(ix), torch.floor(iy)
    out = torch.zeros(P, pts.shape[0], dtype=torch.float64, device=maps.device)
    for dy, wy in ((0, fy + 1.0 - iy), (1, iy - fy)):
        for dx, wx in ((0, fx + 1.0 - ix), (1, ix - fx)):
            xx, yy = fx + dx, fy + dy
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            xi, yi = xx.clamp(0, w - 1).long(), yy.clamp(0, h - 1).long()
            out += m[:, yi, xi] * (wx * wy * ok)[None, :]
    return out, m.abs().amax((1, 2))


# ------------------------------------------------------------------------------ optimizer
def grad_norm_clip(g, pre, max_norm):
    """(|| fl32(g pre) ||_2, min(1, max_norm / (norm + 1e-6)) or 1 for max_norm <= 0) as doubles."""
    v = (g.float() * f32(pre)).double()
    norm = float(torch.sqrt((v * v).sum()))
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    return norm, coef


def adamw_scalars(lr, beta1, beta2, step):
    """The fp32 scalars torch's single-tensor AdamW applies to fp32 tensors, each formed from
    Python doubles: 1 - beta1, 1 - beta2, lr / bc1, sqrt(bc2)."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return f32(1.0 - beta1), f32(1.0 - beta2), f32(lr / bc1), f32(math.sqrt(bc2))


def adamw_step(p, g, m, v, lr, wd, beta1, beta2, eps, step, scalars=f32):
    """One step of torch.optim.AdamW's single-tensor update on float64 copies of (p, m, v) with
    the gradient g; lr / wd: floats or per-element float64 tensors.  `scalars=f32` rounds the
    four scalars as torch does for fp32 tensors; `scalars=float` keeps them double (float64
    parameters).  -> p, m, v and the magnitudes (|m| + |g|, |v| + g^2, the update on absolute
    values)."""
    p64, g64, m64, v64 = p.double(), g.double(), m.double(), v.double()
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    c1, c2, bc2s = scalars(1.0 - beta1), scalars(1.0 - beta2), scalars(math.sqrt(bc2))
    b2s, eps = scalars(beta2), scalars(eps)
    if torch.is_tensor(lr):
        step_size = lr.double() / bc1
        if scalars is f32:
            step_size = step_size.float().double()
    else:
        step_size = scalars(lr / bc1)
    decay = 1.0 - lr * wd
    if scalars is f32:
        decay = decay.float().double() if torch.is_tensor(decay) else f32(decay)
    pd = p64 * decay
    m1 = m64 + (g64 - m64) * c1
    v1 = v64 * b2s + c2 * g64 * g64
    denom = v1.sqrt() / bc2s + eps
    p1 = pd - step_size * (m1 / denom)
    mag_m = m64.abs() + g64.abs()
    mag_d = (p64 - pd).abs() + step_size * ((m64.abs() + (g64.abs() + m64.abs()) * c1) / denom)
    return p1, m1, v1, mag_m, v64.abs() + g64 * g64, mag_d


def segment_layout(nseg, seed):
    """(sizes, offsets [nseg + 1]) of a flat buffer: segment s holds sizes[s] elements from
    offsets[s], zero padding up to offsets[s + 1]; sizes include 1; the last segment ends at
    n = offsets[nseg]."""
    rng = np.random.RandomState(seed)
    sizes = rng.randint(1, 300, size=nseg)
    sizes[0] = 1 if nseg > 1 else 1000
    sizes[-1] = 37 if nseg > 1 else 1000
    if nseg > 2:
        sizes[1] = 4097
    pads = (sizes + 63) // 64 * 64
    pads[-1] = sizes[-1]
    offs = np.concatenate([[0], np.cumsum(pads)]).astype(np.int64)
    return sizes.astype(np.int64), offs
