"""float64 statements of the segmentation-loss kernels (csrc/seg_loss.hip) and of the whole
Mask2Former loss (pair-net_amd/seg_losses.py), written from the formulas in the kernels' headers,
plus the case builders the CPU and GPU tests share.  Every function takes `dtype`: float64 is the
reference, float32 the torch-fp32 oracle whose own error sets the transcendental allowance `a` of
the bounds (labnotes R14.2).  tests/test_seg_loss_refs.py pins the statements (1e-12) to torch's
functions, to `oracle.mmdet_train` and -- where the reference tree is present -- to the reference's
own `loss_single`; tests/test_seg_loss_gpu.py bounds the kernels against them.

[3P] unpinned pieces, restated from memory of mmdet 2.25 like oracle/mmdet_train.py: `DiceLoss`
(`dice_loss` with naive_dice: 1 - (2 sum s t + eps) / (sum s + sum t + eps), then
weight_reduce_loss) and the sigmoid form of `CrossEntropyLoss` (`binary_cross_entropy`:
F.binary_cross_entropy_with_logits(reduction="none") then weight_reduce_loss)."""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

import dropout_ref
import loss_optim_ref as R

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
EPS32 = float(np.finfo(np.float32).eps)

CFG = dict(w_cls=2.0, w_mask=5.0, w_dice=5.0, dice_eps=1.0, c_cls=2.0, c_mask=5.0, c_dice=5.0,
           c_dice_eps=1.0, oversample_ratio=3.0, importance_sample_ratio=0.75)


# ------------------------------------------------------------------------------ uniform draws
def uniform(n, seed, rank, site, step):
    """fp32 [n]: (word >> 8) * 2^-24, word i % 4 of Philox4x32-10 at counter (i / 4, rank, site,
    step), key (seed & 0xffffffff, seed >> 32)."""
    j = np.arange((n + 3) // 4, dtype=np.uint64)
    words = dropout_ref.philox4x32_10((j, rank, site, step),
                                      (seed & dropout_ref.MASK, (seed >> 32) & dropout_ref.MASK))
    w = np.stack(words, axis=1).reshape(-1)[:n]
    return (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


# ------------------------------------------------------------------------------ point sampling
def _taps(pts, h, w, dtype):
    """pts [..., 2] fp32 -> the four (yi, xi, weight, inside) of the bilinear sample, from the fp32
    grid coordinate 2 p - 1 (one rounding, shared with the kernel: loss_optim_ref.point_grid)."""
    c = R.point_grid(pts).to(dtype)
    ix, iy = ((c[..., 0] + 1.0) * w - 1.0) / 2.0, ((c[..., 1] + 1.0) * h - 1.0) / 2.0
    fx, fy = torch.floor(ix), torch.floor(iy)
    out = []
    for dy, wy in ((0, fy + 1.0 - iy), (1, iy - fy)):
        for dx, wx in ((0, fx + 1.0 - ix), (1, ix - fx)):
            xx, yy = fx + dx, fy + dy
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            out.append((yy.clamp(0, h - 1).long(), xx.clamp(0, w - 1).long(), wx * wy, ok))
    return out


def sample_rows(maps, idx, pts, dtype=torch.float64):
    """Row m: map idx[m] of maps [n][h][w] at pts [M][Np][2] -> [M][Np]; idx < 0: zeros.
    Differentiable in `maps`."""
    n, h, w = maps.shape
    idx = torch.as_tensor(idx, dtype=torch.int64)
    m = maps.to(dtype)
    out = torch.zeros(pts.shape[:2], dtype=dtype)
    rows = idx.clamp(min=0)[:, None].expand(pts.shape[:2])
    for yi, xi, wt, ok in _taps(pts, h, w, dtype):
        out = out + m[rows, yi, xi] * (wt * ok)
    return out * (idx >= 0)[:, None]


def sample_mag(maps, idx):
    """R14.2's magnitude of a point sample: (1 + max(h, w)) * max |tap| of the row's map."""
    n, h, w = maps.shape
    idx = torch.as_tensor(idx, dtype=torch.int64)
    big = maps.double().abs().amax((1, 2))
    return (1.0 + max(h, w)) * big[idx.clamp(min=0)] * (idx >= 0)


# Absolute error of a tap weight in roundings (2^-24) of max(h, w): the pixel coordinate
# ix = ((2 p - 1 + 1) n - 1) / 2 carries the roundings of 2 p - 1 (half an ulp below 1: n / 2), of
# the sum below 2 (n), of the product below 2 n (n) and of the difference (n), the halving is exact:
# <= 3.5 n; a weight factor fx + 1 - ix adds its own rounding of a value <= 1; the product of two
# factors <= 1 carries both: <= 2 * 3.5 max(h, w) + 3 <= COORD (1 + max(h, w)).
COORD = 8.0


def sample_err(maps, idx, pts):
    """Per-point bound of a sample's fp32 error, [M][Np]: 6 roundings of the sum on absolute values
    (weight product, tap product, four additions) + COORD (1 + max(h, w)) roundings of the largest of
    the four taps the point reads -- local, where sample_mag takes the map's largest tap."""
    n, h, w = maps.shape
    idx = torch.as_tensor(idx, dtype=torch.int64)
    m = maps.double().abs()
    rows = idx.clamp(min=0)[:, None].expand(pts.shape[:2])
    mag = torch.zeros(pts.shape[:2], dtype=torch.float64)
    big = torch.zeros(pts.shape[:2], dtype=torch.float64)
    for yi, xi, wt, ok in _taps(pts, h, w, torch.float64):
        tap = m[rows, yi, xi] * ok
        mag, big = mag + tap * wt, torch.maximum(big, tap)
    return U * (6.0 * mag + COORD * (1.0 + max(h, w)) * big) * (idx >= 0)[:, None]


def exact_centres(h, w):
    """Pixels whose centre (j + 0.5) / n is exact in fp32 AND stays exact through 2 p - 1 and the
    un-normalisation (R14.2's rule): returns ([ys], [xs])."""
    def axis(n):
        return [j for j in range(n)
                if float(np.float32((j + 0.5) / n)) * n == j + 0.5]
    return axis(h), axis(w)


def scatter(coef, pts, h, w, dtype=torch.float64):
    """The transpose of sample_rows: [M][Np] coefficients -> ([M][h][w], mag, contributions per
    pixel, coord).  mag is the computation on absolute values, sum |coef * weight|.  coord carries
    what mag cannot: a tap weight is a product of differences of coordinates of size up to
    max(h, w), so it has an ABSOLUTE error however small it is (COORD roundings of max(h, w), see
    COORD below): coord = (1 + max(h, w)) * the sum of |coef| over the points with a tap on the
    pixel, to be used with the constant COORD, beside and not times the chain's c."""
    M, Np = coef.shape
    c = coef.to(dtype)
    out = torch.zeros(M, h * w, dtype=dtype)
    mag = torch.zeros(M, h * w, dtype=dtype)
    cnt = torch.zeros(M, h * w, dtype=dtype)
    coord = torch.zeros(M, h * w, dtype=dtype)
    for yi, xi, wt, ok in _taps(pts, h, w, dtype):
        flat = yi * w + xi
        out.scatter_add_(1, flat, c * wt * ok)
        mag.scatter_add_(1, flat, (c * wt * ok).abs())
        coord.scatter_add_(1, flat, (1.0 + max(h, w)) * (c * ok).abs())
        cnt.scatter_add_(1, flat, ok.to(dtype))
    return out.view(M, h, w), mag.view(M, h, w), cnt.view(M, h, w), coord.view(M, h, w)


# ------------------------------------------------------------------------------ selection
def uncertain_points(maps, idx, cand, tail, k, dtype=torch.float64):
    """point_sample.py:32-88 per row: the k candidates with the smallest |logit| (stable: ties to
    the lower index) in ascending candidate order, then the tail.  -> (pts [M][Np][2], kept index
    sets [M][k] ascending, |logit| [M][S])."""
    key = sample_rows(maps, idx, cand, dtype).abs()
    order = torch.sort(key, dim=1, stable=True)[1][:, :k]
    kept = torch.sort(order, dim=1)[0]
    sel = torch.gather(cand, 1, kept[:, :, None].expand(-1, -1, 2))
    pts = sel if tail is None else torch.cat([sel, tail.to(cand.dtype)], 1)
    return pts, kept, key


# ------------------------------------------------------------------------------ point losses
def bce(x, t):
    """F.binary_cross_entropy_with_logits(x, t, reduction="none") written out."""
    return torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))


def mask_point_loss(x, t, valid, L, w_mask, w_dice, eps, ntm=None, dtype=torch.float64):
    """x / t [M][Np], M = L * Ml rows in table order, valid [M] bool -> dict(mask [L], dice [L],
    mask_mag, dice_mag, sums [M][4], den [L][2]).  Differentiable in x."""
    M, Np = x.shape
    Ml = M // L
    x, t = x.to(dtype), t.to(dtype)
    v = torch.as_tensor(valid).to(dtype)
    s = torch.sigmoid(x)
    b_m, a, b, c = bce(x, t).sum(1), (s * t).sum(1), s.sum(1), t.sum(1)
    b_abs = (torch.clamp(x, min=0) + (x * t).abs() + torch.log1p(torch.exp(-x.abs()))).sum(1)
    frac = (2.0 * a + eps) / (b + c + eps)
    cnt = v.view(L, Ml).sum(1)
    N = torch.clamp(cnt, min=1.0) if ntm is None else torch.full_like(cnt, float(ntm))
    if dtype == torch.float32:
        den_m, den_d = N * np.float32(Np) + np.float32(EPS32), N + np.float32(EPS32)
    else:
        den_m, den_d = N * Np + EPS32, N + EPS32
    lm = w_mask * ((b_m * v).view(L, Ml).sum(1) / den_m)
    ld = w_dice * (((1.0 - frac) * v).view(L, Ml).sum(1) / den_d)
    return dict(mask=lm, dice=ld, mask_mag=w_mask * ((b_abs * v).view(L, Ml).sum(1) / den_m),
                dice_mag=w_dice * (((1.0 + frac) * v).view(L, Ml).sum(1) / den_d),
                sums=torch.stack([b_m, a, b, c], 1), den=torch.stack([den_m, den_d], 1))


def mask_point_coef(x, t, valid, L, w_mask, w_dice, eps, ntm=None, dtype=torch.float64):
    """d (sum of the 2L terms) / d x by autograd through mask_point_loss -> (coef [M][Np], the
    analytic expression on absolute values)."""
    xx = x.detach().to(dtype).requires_grad_(True)
    with torch.enable_grad():
        r = mask_point_loss(xx, t, valid, L, w_mask, w_dice, eps, ntm, dtype)
        (r["mask"].sum() + r["dice"].sum()).backward()
    with torch.no_grad():
        M, Np = x.shape
        s, tt = torch.sigmoid(xx), t.to(dtype)
        sm = r["sums"]
        num, den = (2.0 * sm[:, 1] + eps)[:, None], (sm[:, 2] + sm[:, 3] + eps)[:, None]
        lay = torch.arange(M) // (M // L)
        dm, dd = r["den"][lay, 0][:, None], r["den"][lay, 1][:, None]
        mag = w_mask * (s + tt) / dm + (w_dice / dd) * ((num + 2.0 * tt * den) / (den * den)) * s * (1.0 - s)
        mag = mag * torch.as_tensor(valid).to(dtype)[:, None]
    return xx.grad.detach(), mag


# ------------------------------------------------------------------------------ loss_cls
def ce_avg(x, y, cw, lw, dtype=torch.float64):
    """x [L][rows][C], y [L][rows], cw [C] -> (out [L], mag [L]); differentiable in x."""
    x, cw = x.to(dtype), torch.as_tensor(cw).to(dtype)
    lse = torch.logsumexp(x, -1)
    xy = torch.gather(x, 2, y[:, :, None])[:, :, 0]
    wy = cw[y]
    den = wy.sum(1) + (np.float32(EPS32) if dtype == torch.float32 else EPS32)
    return lw * ((wy * (lse - xy)).sum(1) / den), lw * ((wy * (lse.abs() + xy.abs())).sum(1) / den)


def ce_avg_grad(x, y, cw, lw, dtype=torch.float64):
    xx = x.detach().to(dtype).requires_grad_(True)
    with torch.enable_grad():
        ce_avg(xx, y, cw, lw, dtype)[0].sum().backward()
    with torch.no_grad():
        wy = torch.as_tensor(cw).to(dtype)[y]
        den = wy.sum(1, keepdim=True) + EPS32
        onehot = F.one_hot(y, x.shape[-1]).to(dtype)
        mag = lw * (wy / den)[:, :, None] * (torch.softmax(xx, -1) + onehot)
    return xx.grad.detach(), mag


# ------------------------------------------------------------------------------ the whole loss
def whole_loss(cls, mask, gt_labels, gt_masks, points, num_classes, class_weight, num_points,
               cfg=CFG, dtype=torch.float64, ntm=None, assignment=None, grad=True):
    """The Mask2Former loss of seg_losses.py in `dtype` from fp32 inputs: cls [L][B][Q][C+1], mask
    [L][B][Q][h][w], per image gt_labels [G] / gt_masks [G][hg][wg] 0/1 (their own grid); points = dict(assign=[L][B]
    of [Np][2], and candidates / tail per layer or loss per layer).  `assignment`: {(l, b): (rows,
    cols)} to bypass scipy; `grad=False`: values only (no g_* / *_mag entries).  -> dict(losses={name: 0-dim}, g_cls, mask_rows [M], g_mask [M][h][w],
    matched [M][4], labels [L][B*Q], pts [M][Np][2], costs {(l, b): float64 cost matrix},
    mags={name: the term on absolute values}, g_cls_mag, g_mask_mag [M][h][w])."""
    L, B, Q, C1 = cls.shape
    h, w = mask.shape[-2:]
    cls_v = cls.detach().to(dtype).requires_grad_(grad)
    mask_v = mask.detach().to(dtype).requires_grad_(grad)
    maps = mask_v.view(L * B * Q, h, w)
    G = [int(g.shape[0]) for g in gt_labels]
    goff = np.concatenate([[0], np.cumsum(G)])
    gt_all = torch.cat([torch.as_tensor(m).to(dtype) for m in gt_masks if m.shape[0]]) \
        if sum(G) else torch.zeros(1, h, w, dtype=dtype)
    labels = torch.full((L, B * Q), num_classes, dtype=torch.int64)
    matched, costs = [], {}
    with torch.no_grad():
        for l in range(L):
            for b in range(B):
                if G[b] == 0:
                    continue
                if assignment is not None:
                    rows, cols = assignment[(l, b)]
                else:
                    pts = torch.as_tensor(points["assign"][l][b]).reshape(1, -1, 2).float()
                    qi = torch.arange(Q) + (l * B + b) * Q
                    x = sample_rows(maps, qi, pts.expand(Q, -1, -1), dtype)
                    t = sample_rows(gt_all, torch.arange(G[b]) + goff[b], pts.expand(G[b], -1, -1),
                                    dtype)
                    gl = torch.as_tensor(gt_labels[b]).long()
                    if dtype == torch.float64:
                        cost = R.mask_match_cost(cls[l, b], gl, x, t, cfg["c_cls"], cfg["c_mask"],
                                                 cfg["c_dice"], cfg["c_dice_eps"])[0]
                    else:
                        cost = _match_cost32(cls[l, b], gl, x, t, cfg)
                    costs[(l, b)] = cost
                    rows, cols = linear_sum_assignment(cost.numpy())
                order = np.argsort(rows)
                for q, g in zip(np.asarray(rows)[order], np.asarray(cols)[order]):
                    labels[l, b * Q + q] = int(gt_labels[b][g])
                    matched.append((l, b, int(q), int(goff[b] + g)))
    matched = torch.tensor(matched, dtype=torch.int64).reshape(-1, 4)
    M = matched.shape[0]
    l_cls, m_cls = ce_avg(cls_v.view(L, B * Q, C1), labels, class_weight, cfg["w_cls"], dtype)
    out = dict(labels=labels, matched=matched)
    m_mask = m_dice = torch.zeros(L, dtype=dtype)
    g_mask_mag = g_mask_coord = torch.zeros(0, h, w, dtype=dtype)
    rows_idx = (matched[:, 0] * B + matched[:, 1]) * Q + matched[:, 2]
    if M == 0:
        lm = ld = torch.zeros(L, dtype=dtype)
        pts = torch.zeros(0, num_points, 2)
    else:
        Ml = M // L
        if "loss" in points:
            pts = torch.cat([torch.as_tensor(p).float().reshape(Ml, -1, 2) for p in points["loss"]])
        else:
            cand = torch.cat([torch.as_tensor(p).float().reshape(Ml, -1, 2)
                              for p in points["candidates"]])
            k = int(cfg["importance_sample_ratio"] * num_points)
            tail = torch.cat([torch.as_tensor(p).float().reshape(Ml, -1, 2)
                              for p in points["tail"]]) if k < num_points else None
            with torch.no_grad():
                pts, kept, key = uncertain_points(maps.detach(), rows_idx, cand, tail, k, dtype)
            out.update(kept=kept, key=key)
        x = sample_rows(maps, rows_idx, pts, dtype)
        t = sample_rows(gt_all, matched[:, 3], pts, dtype)
        r = mask_point_loss(x, t, torch.ones(M, dtype=torch.bool), L, cfg["w_mask"], cfg["w_dice"],
                            cfg["dice_eps"], ntm, dtype)
        lm, ld = r["mask"], r["dice"]
        m_mask, m_dice = r["mask_mag"].detach(), r["dice_mag"].detach()
        if grad:
            cmag = mask_point_coef(x.detach(), t.detach(), torch.ones(M, dtype=torch.bool), L,
                                   cfg["w_mask"], cfg["w_dice"], cfg["dice_eps"], ntm, dtype)[1]
            sc = scatter(cmag, pts, h, w, dtype)
            g_mask_mag, g_mask_coord = sc[1], sc[3]
        out.update(x=x.detach(), t=t.detach())
    losses = dict(loss_cls=l_cls[L - 1], loss_mask=lm[L - 1], loss_dice=ld[L - 1])
    for l in range(L - 1):
        losses["d%d.loss_cls" % l], losses["d%d.loss_mask" % l] = l_cls[l], lm[l]
        losses["d%d.loss_dice" % l] = ld[l]
    mags = dict(loss_cls=m_cls[L - 1], loss_mask=m_mask[L - 1], loss_dice=m_dice[L - 1])
    for l in range(L - 1):
        mags["d%d.loss_cls" % l], mags["d%d.loss_mask" % l] = m_cls[l], m_mask[l]
        mags["d%d.loss_dice" % l] = m_dice[l]
    out.update(mags={k: v.detach() for k, v in mags.items()},
               losses={k: v.detach() for k, v in losses.items()}, mask_rows=rows_idx, pts=pts,
               costs=costs)
    if grad:
        (l_cls.sum() + lm.sum() + ld.sum()).backward()
        g_mask = mask_v.grad if mask_v.grad is not None else torch.zeros_like(mask_v)
        g_cls_mag = ce_avg_grad(cls.view(L, B * Q, C1), labels, class_weight, cfg["w_cls"],
                                dtype)[1].view(L, B, Q, C1)
        out.update(g_cls=cls_v.grad.detach(), g_cls_mag=g_cls_mag, g_mask_mag=g_mask_mag, g_mask_coord=g_mask_coord,
                   g_mask=g_mask.view(L * B * Q, h, w)[rows_idx].detach())
    return out


def _match_cost32(cls, labels, x, t, cfg):
    """The same cost in torch fp32 (the oracle's arithmetic of oracle.mmdet_train's three costs)."""
    Np = x.shape[1]
    c_cls = -torch.softmax(cls, -1)[:, labels] * cfg["c_cls"]
    pos = F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
    neg = F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
    c_mask = (pos @ t.T + neg @ (1 - t).T) / Np * cfg["c_mask"]
    s = torch.sigmoid(x)
    c_dice = (1 - (2 * (s @ t.T) + cfg["c_dice_eps"])
              / (s.sum(-1)[:, None] + t.sum(-1)[None, :] + cfg["c_dice_eps"])) * cfg["c_dice"]
    return c_cls + c_mask + c_dice


# ------------------------------------------------------------------------------ case builders
def loss_case(L, B, Q, C, h, w, Np, G, seed, oversample=3.0, ratio=0.75):
    """Seeded inputs of one whole-loss case with a planted assignment: in every layer, ground
    truth g of image b is matched by query (3 g + l + b) % Q -- that query's mask logits follow the
    ground-truth mask (+-4 plus noise) and its class logit leads by 6 -- so the assigned entry of
    every cost row leads by far more than the cost kernels' error (checked on the CPU in
    tests/test_seg_loss_refs.py).  Ground-truth masks are random rectangles, mask 0 of an image
    with G >= 2 is empty.  -> dict(cls, mask, gt_labels, gt_masks, points, planted)."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(L, B, Q, C + 1, generator=g) * 2.0
    mask = torch.randn(L, B, Q, h, w, generator=g) * 2.0
    gt_labels, gt_masks, planted = [], [], {}
    for b in range(B):
        gl = torch.randint(0, C, (G[b],), generator=g)
        gm = torch.zeros(G[b], h, w, dtype=torch.uint8)
        for j in range(G[b]):
            y0, x0 = int(torch.randint(0, h - 1, (1,), generator=g)), int(torch.randint(0, w - 1, (1,), generator=g))
            y1, x1 = int(torch.randint(y0 + 1, h + 1, (1,), generator=g)), int(torch.randint(x0 + 1, w + 1, (1,), generator=g))
            if not (j == 0 and G[b] >= 2):
                gm[j, y0:y1, x0:x1] = 1
        gt_labels.append(gl)
        gt_masks.append(gm)
        n = min(Q, G[b])
        for l in range(L):
            qs = [(3 * j + l + b) % Q for j in range(n)]
            assert len(set(qs)) == n, "planted queries collide: choose Q coprime to 3 or larger"
            for j, q in enumerate(qs):
                mask[l, b, q] = (gm[j].float() * 8.0 - 4.0) + 0.5 * torch.randn(h, w, generator=g)
                cls[l, b, q, gl[j]] += 6.0
            planted[(l, b)] = sorted(zip(qs, range(n)))
    Ml = sum(min(Q, x) for x in G)
    S, k = int(Np * oversample), int(ratio * Np)
    points = dict(assign=[[torch.rand(Np, 2, generator=g) for _ in range(B)] for _ in range(L)],
                  candidates=[torch.rand(Ml, S, 2, generator=g) for _ in range(L)],
                  tail=[torch.rand(Ml, Np - k, 2, generator=g) for _ in range(L)])
    return dict(cls=cls, mask=mask, gt_labels=gt_labels, gt_masks=gt_masks, points=points,
                planted=planted, num_classes=C, num_points=Np,
                class_weight=[1.0] * C + [0.1])


def selection_case(M, h, w, S, seed, mode="random"):
    """maps [M][h][w] and candidates [M][S][2] of one selection case.  mode "equal": every logit of
    row 0's map is the same; "pairs": row 0's map holds +-v pairs of equal magnitude."""
    g = torch.Generator().manual_seed(seed)
    maps = torch.randn(M, h, w, generator=g) * 3.0
    cand = torch.rand(M, S, 2, generator=g)
    if mode == "equal":
        maps[0] = 0.0                        # (every sample is exactly 0: the keys ARE equal)
    if mode == "pairs":
        v = torch.randn(h, (w + 1) // 2, generator=g)
        maps[0] = torch.cat([v, -v], 1)[:, :w]
    return maps, cand


# ------------------------------------------------------------------------------ shared cases
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_loss.npz")
# whole-loss cases drawn here (the fixture's two are "a" and "b"): 18 problems in one launch; more
# ground truth than queries on one image; no ground truth at all
WHOLE_CASES = dict(l9=dict(L=9, B=2, Q=8, C=5, h=13, w=21, Np=50, G=(3, 2), seed=21),
                   g_gt_q=dict(L=2, B=2, Q=4, C=5, h=13, w=21, Np=50, G=(6, 2), seed=22),
                   empty=dict(L=2, B=2, Q=8, C=5, h=13, w=21, Np=50, G=(0, 0), seed=23))
# selection cases (M 5, 13 x 21) whose fp32 torch run keeps the float64 run's k-set (asserted on the
# CPU): (S, k, seed)
SELECTION_CASES = [(150, 37, 1), (192, 48, 2), (3, 0, 3), (4, 4, 4), (150, 150, 5)]


def golden_case(name):
    """Fixture case "a" / "b" -> (a loss_case-shaped dict, the stored reference values)."""
    z = np.load(GOLDEN)
    pre = name + "."
    L, B, Q, C, h, w, Np = (int(v) for v in z[pre + "shape"])
    T = lambda k: torch.from_numpy(z[pre + k])
    case = dict(cls=T("cls"), mask=T("mask"), gt_labels=[T("gt_labels.%d" % b) for b in range(B)],
                gt_masks=[T("gt_masks.%d" % b) for b in range(B)], num_classes=C, num_points=Np,
                class_weight=[1.0] * C + [0.1],
                points=dict(assign=[[T("assign.%d.%d" % (l, b)) for b in range(B)] for l in range(L)],
                            candidates=[T("candidates.%d" % l) for l in range(L)],
                            tail=[T("tail.%d" % l) for l in range(L)]))
    ref = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    return case, ref


def run_whole(case, dtype=torch.float64, points=None, **kw):
    return whole_loss(case["cls"], case["mask"], case["gt_labels"], case["gt_masks"],
                      points or case["points"], case["num_classes"], case["class_weight"],
                      case["num_points"], dtype=dtype, **kw)


# ------------------------------------------------------------------------------ the reference itself
# Executed in place from its own tree (present on build machines only), under name-only stubs; the
# [3P] pieces it calls and the oracle does not carry are restated here from memory, unpinned.
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class SigmoidCE:
    """[3P] mmdet CrossEntropyLoss(use_sigmoid=True), for equal-shaped float targets."""

    def __init__(self, loss_weight):
        self.loss_weight = loss_weight

    def __call__(self, pred, target, avg_factor=None):
        from oracle.mmdet_train import weight_reduce_loss
        loss = F.binary_cross_entropy_with_logits(pred, target.to(pred.dtype), reduction="none")
        return self.loss_weight * weight_reduce_loss(loss, None, "mean", avg_factor)


class DiceLoss:
    """[3P] mmdet DiceLoss(use_sigmoid=True, activate=True, naive_dice=True)."""

    def __init__(self, loss_weight, eps):
        self.loss_weight, self.eps = loss_weight, eps

    def __call__(self, pred, target, avg_factor=None):
        from oracle.mmdet_train import weight_reduce_loss
        s, t = pred.sigmoid().flatten(1), target.flatten(1).to(pred.dtype)
        a, b, c = torch.sum(s * t, 1), torch.sum(s, 1), torch.sum(t, 1)
        loss = 1 - (2 * a + self.eps) / (b + c + self.eps)
        return self.loss_weight * weight_reduce_loss(loss, None, "mean", avg_factor)


def load_reference():
    """The reference's Mask2FormerHead class, loaded in place under name-only stubs."""
    from oracle import ref_shim
    name = "pairnet.models.panoptic_heads.mask2former_head"
    if name in sys.modules:
        return sys.modules[name].Mask2FormerHead
    ref_shim.install_training()
    sys.modules["mmdet.core"].reduce_mean = lambda t: t
    ref_shim._mod("mmdet.models.dense_heads.anchor_free_head",
                  AnchorFreeHead=sys.modules["mmdet.models.dense_heads"].AnchorFreeHead)
    ref_shim._mod("pairnet.models.panoptic_heads")
    ref_shim._mod("pairnet.models.panoptic_heads.panoptic_gt_processing", preprocess_panoptic_gt=None)
    for m in ("point_sample", "maskformer_head", "mask2former_head"):
        ref_shim._load("pairnet.models.panoptic_heads." + m, "pairnet/models/panoptic_heads/%s.py" % m)
    return sys.modules[name].Mask2FormerHead


@contextlib.contextmanager
def injected_rand(draws, dtype):
    """`torch.rand` hands out `draws` in order (shape-checked), as the reference would draw them."""
    real, queue = torch.rand, list(draws)

    def fake(*size, **kw):
        size = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        t = queue.pop(0)
        assert tuple(t.shape) == size, (tuple(t.shape), size)
        return t.to(dtype)
    torch.rand = fake
    try:
        yield
    finally:
        torch.rand = real
    assert not queue, "%d draws left over" % len(queue)


def run_reference(case, dtype=torch.float32, cfg=None):
    """`MaskFormerHead.loss` of the reference on a seg_loss_ref.loss_case -> (loss dict, d sum / d
    cls, d sum / d mask), in `dtype`."""
    from oracle import mmdet_train as T
    cfg = cfg or CFG
    Head = load_reference()
    head = Head.__new__(Head)
    L, B, Q = case["cls"].shape[:3]
    Np = case["num_points"]
    # (the class weights are fp32 data, like the logits: a float64 run starts from their fp32 values)
    cw = [float(np.float32(v)) for v in case["class_weight"]]
    attrs = dict(num_points=Np, num_queries=Q, num_classes=case["num_classes"], class_weight=cw, oversample_ratio=cfg["oversample_ratio"],
                 importance_sample_ratio=cfg["importance_sample_ratio"],
                 assigner=T.build_assigner(dict(
                     type="MaskHungarianAssigner",
                     cls_cost=dict(type="ClassificationCost", weight=cfg["c_cls"]),
                     mask_cost=dict(type="CrossEntropyLossCost", weight=cfg["c_mask"], use_sigmoid=True),
                     dice_cost=dict(type="DiceCost", weight=cfg["c_dice"], pred_act=True,
                                    eps=cfg["c_dice_eps"]))),
                 sampler=T.build_sampler(dict(type="MaskPseudoSampler")),
                 loss_cls=T.CrossEntropyLoss(use_sigmoid=False, loss_weight=cfg["w_cls"],
                                             reduction="mean", class_weight=cw),
                 loss_mask=SigmoidCE(cfg["w_mask"]), loss_dice=DiceLoss(cfg["w_dice"], cfg["dice_eps"]))
    for k, v in attrs.items():
        object.__setattr__(head, k, v)
    pts, G = case["points"], [int(g.shape[0]) for g in case["gt_labels"]]
    Ml = sum(min(Q, g) for g in G)
    k = int(cfg["importance_sample_ratio"] * Np)
    draws = []
    for l in range(L):        # the order of the reference's torch.rand calls
        draws += [pts["assign"][l][b].reshape(1, -1, 2) for b in range(B)]
        if Ml:
            draws.append(pts["candidates"][l])
            if k < Np:
                draws.append(pts["tail"][l])
    cls = case["cls"].detach().clone().to(dtype).requires_grad_(True)
    mask = case["mask"].detach().clone().to(dtype).requires_grad_(True)
    real_float = torch.Tensor.float
    if dtype == torch.float64:       # the reference's `.float()` casts follow the run's precision
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        with injected_rand(draws, dtype):
            out = _loss(head, cls, mask, case, dtype, B)
    finally:
        torch.Tensor.float = real_float
    sum(out.values()).backward()
    g_mask = mask.grad if mask.grad is not None else torch.zeros_like(mask)
    return {k: v.detach() for k, v in out.items()}, cls.grad.detach(), g_mask.detach()


def _loss(head, cls, mask, case, dtype, B):
    return head.loss(cls, mask, [g.long() for g in case["gt_labels"]],
                     [m.to(dtype) for m in case["gt_masks"]], [dict() for _ in range(B)])
