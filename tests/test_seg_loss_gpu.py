"""GPU: every kernel of csrc/seg_loss.hip alone, and the whole Mask2Former loss
(pair-net_amd/seg_losses.py), against the float64 statements of tests/seg_loss_ref.py and the
fixture tests/golden/seg_loss.npz (recorded from the reference's own loss).

Bound form (labnotes R14.2): |got - ref64| <= c * 2^-24 * mag + FLT_MIN per element, c = L_chain + a.
`mag` is the float64 computation on absolute values; `a`, the allowance for expf / logf / log1pf /
division, is twice the ratio the torch-fp32 run of the same statement reaches against its float64
run on the same inputs, and at least 4.  Nothing in c is measured from the kernel under test.
L_chain, counted from the source, with K = ceil(Np / 256) + 10 (a thread's strided sum, 6 wave
steps, 4 waves):

  k_point_sample_rows   14 (two coordinates 6, weights 3, tap 1, four additions; R14.2's count for
                        k_point_sample, whose arithmetic it repeats); mag (1 + max(h, w)) max|tap|
  k_mask_point_sums /   loss_mask: K + 4 (the BCE element) + Ml (serial sum over the layer's masks)
  k_mask_point_finish   + 4 (N Np, + eps32, quotient, weight);
                        loss_dice: 2 K + 10 (a, b, c each K + 2 with the sigmoid's two; 2a + eps and
                        b + c + eps two each; quotient; 1 - frac) + Ml + 4; mag (1 + frac)
  k_mask_point_coef     4 K + 34: the BCE part 8 (sigmoid 3, s - t, the denominator's 3, quotient),
                        the dice part num K + 4, den K + 5 and den^2 2 K + 9, the difference and the
                        quotient 2, s (1 - s) 6, two products, w / den 4, the final sum 1
  k_point_scatter_grad  n + 15 for a pixel with n contributions (weight 14, product 1, n additions)
                        on mag = sum |coef * weight|; BESIDE it, not times it, the tap weights'
                        coordinate error: COORD = 8 roundings of (1 + max(h, w)) sum |coef|
                        (seg_loss_ref.COORD: a weight is a product of coordinate differences of size
                        max(h, w) and has an absolute error however small it is -- torch's own fp32
                        autograd through grid_sample misses mag alone by thousands of roundings)
  k_ce_avg              ceil(C / 64) + 2 rows + 14 + ceil(ln C + 1) (k_ce_mean's count, R14.2, with
                        the second serial sum of the denominator)
  k_ce_avg_grad         rows + ceil(C / 64) + 14 + z, z = min(88, max x - x[c]) per element (R14.2)

The whole loss chains these kernels, so its bound adds what the samples' own error (per point:
seg_loss_ref.sample_err, 6 roundings of the sample on absolute values + COORD roundings of
(1 + max(h, w)) times the largest of the four taps the point reads) does to each output, to first
order, through the float64 statement's own derivatives:
sum |d out / d x| dx + sum |d out / d t| dt (autograd in float64; nothing from the kernels)."""
import math

import numpy as np
import pytest
import torch

import seg_loss_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U, FLT_MIN = S.U, S.FLT_MIN
WORST = {}


def _hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip
    return hip


def _ratio(name, got, ref, mag, c):
    """Assert the bound elementwise; record and print the worst |err| / (2^-24 mag)."""
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    ref, mag = torch.as_tensor(ref).double().reshape(-1), torch.as_tensor(mag).double().reshape(-1)
    c = torch.as_tensor(c, dtype=torch.float64).reshape(-1)
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    ratio = float((err / (U * mag + FLT_MIN)).max()) if err.numel() else 0.0
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print("%s: worst ratio %.3f (c >= %.1f)" % (name, ratio, float(c.min()) if c.numel() else 0))
    bad = err > c * U * mag + FLT_MIN
    assert not bool(bad.any()), (name, ratio, float(c.min()))
    return ratio


def _allow(v32, v64, mag):
    """a: twice the torch-fp32 oracle's own ratio, at least 4."""
    r = ((torch.as_tensor(v32).double() - torch.as_tensor(v64).double()).abs()
         / (U * torch.as_tensor(mag).double() + FLT_MIN))
    return max(4.0, 2.0 * float(r.max())) if r.numel() else 4.0


def _dev(t):
    return t.to(DEV).contiguous()


# ------------------------------------------------------------------------------ uniform
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099])
def test_uniform_equals_the_host_philox_bit_for_bit(n):
    hip = _hip()
    seed, rank, site, step = 0x123456789ABCDEF, 3, 7, 11
    out = torch.full((2, n), -1.0, device=DEV)
    hip.uniform(out, seed, rank, step, site, site_stride=4)
    got = out.cpu().numpy()
    for s in range(2):
        assert np.array_equal(got[s], S.uniform(n, seed, rank, site + 4 * s, step))
    assert (got >= 0).all() and (got < 1).all()
    if n >= 4:
        for other in ((1, rank, step, site), (seed, 4, step, site), (seed, rank, 12, site),
                      (seed, rank, step, 8)):
            o2 = torch.empty(n, device=DEV)
            hip.uniform(o2, *other)
            assert not np.array_equal(o2.cpu().numpy(), got[0])
    again = torch.empty(2, n, device=DEV)
    hip.uniform(again, seed, rank, step, site, site_stride=4)
    assert torch.equal(again, out)


# ------------------------------------------------------------------------------ row point sample
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (13, 21), (200, 334)])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("Np", [1, 50, 257])
def test_point_sample_rows(h, w, u8, Np):
    hip = _hip()
    g = torch.Generator().manual_seed(h * 1000 + w + Np)
    maps = (torch.rand(4, h, w, generator=g) > 0.5).to(torch.uint8) if u8 else \
        torch.randn(4, h, w, generator=g) * 3.0
    idx = torch.tensor([2, 2, 0, -1, 3, 0])                  # repeats, skips map 1, one empty row
    ys, xs = S.exact_centres(h, w)
    assert ys and xs
    pts = torch.rand(6, Np, 2, generator=g)
    below1 = float(np.nextafter(np.float32(1), np.float32(0)))
    special = [(0.0, 0.0), (below1, below1), (0.0, below1)] + \
        [((x + 0.5) / w, (y + 0.5) / h) for y in ys[:2] for x in xs[:2]]
    n_sp = min(len(special), Np)
    pts[:, :n_sp] = torch.tensor(special[:n_sp], dtype=torch.float32)
    out = torch.full((6, Np), float("nan"), device=DEV)
    hip.point_sample_rows(_dev(maps), _dev(idx), _dev(pts), out)
    ref = S.sample_rows(maps, idx, pts)
    _ratio("k_point_sample_rows", out, ref, S.sample_mag(maps, idx)[:, None].expand(-1, Np), 14 + 4)
    assert float(out[3].abs().max()) == 0.0
    got = out.cpu()
    for j in range(3, n_sp):         # exact pixel centres: the pixel itself, exactly
        x, y = round(special[j][0] * w - 0.5), round(special[j][1] * h - 0.5)
        for r in (0, 1, 2, 4, 5):
            assert float(got[r, j]) == float(maps[idx[r], y, x]), (r, j)


# ------------------------------------------------------------------------------ selection
def _select(maps, cand, k, Np, tail):
    hip = _hip()
    M, Sn, _ = cand.shape
    matched = torch.stack([torch.zeros(M), torch.zeros(M), torch.arange(M), torch.zeros(M)], 1).long()
    keys = torch.full((M, Sn), -1, dtype=torch.int32, device=DEV)
    pts = torch.full((M, Np, 2), float("nan"), device=DEV)
    hip.uncertain_points(_dev(maps), _dev(matched), 1, M, _dev(cand), None if tail is None else _dev(tail),
                         k, keys, pts)
    return keys.cpu().view(torch.float32), pts.cpu()


def _check_selection(maps, cand, k, Np, tail, separated):
    M, Sn, _ = cand.shape
    key, pts = _select(maps, cand, k, Np, tail)
    idx = torch.arange(M)
    # the kept set is torch.topk of the kernel's OWN |x| (stable: ties to the lower index),
    # in ascending candidate order -- exactly and always
    own = torch.sort(torch.sort(key, dim=1, stable=True)[1][:, :k], 1)[0]
    assert torch.equal(pts[:, :k], torch.gather(cand, 1, own[:, :, None].expand(-1, -1, 2)))
    if k:
        top = torch.topk(-key, k, dim=1)[1]
        kth = -torch.topk(-key, k, dim=1)[0][:, -1:]
        assert bool((torch.gather(key, 1, own) <= kth).all()) and bool((torch.gather(key, 1, top) <= kth).all())
    if tail is not None:
        assert torch.equal(pts[:, k:], tail)
    ref_pts, ref_kept, ref_key = S.uncertain_points(maps, idx, cand, tail, k)
    bound = 18 * U * S.sample_mag(maps, idx)[:, None] + FLT_MIN
    assert bool(((key.double() - ref_key).abs() <= bound).all())
    if separated:
        assert torch.equal(own, ref_kept)
    elif 0 < k < Sn:
        kth64 = torch.sort(ref_key, 1)[0][:, k - 1:k]
        for m in range(M):
            diff = set(own[m].tolist()) ^ set(ref_kept[m].tolist())
            # a swapped candidate lies within TWICE the sample bound of the float64 k-th value: its own
            # key is off by one bound, and the kernel's k-th value is off by one bound from the float64 one
            for i in diff:
                assert abs(float(ref_key[m, i] - kth64[m, 0])) <= 2 * float(bound[m, 0]), (m, i)
    return own


@pytest.mark.parametrize("Sn,k,seed", S.SELECTION_CASES)
def test_selection_small_cases(Sn, k, seed):
    maps, cand = S.selection_case(5, 13, 21, Sn, seed)
    Np = {(150, 37): 50, (192, 48): 64, (3, 0): 1, (4, 4): 4, (150, 150): 150}[(Sn, k)]
    tail = torch.rand(5, Np - k, 2, generator=torch.Generator().manual_seed(seed)) if k < Np else None
    _check_selection(maps, cand, k, Np, tail, separated=True)


def test_selection_ties_take_the_lower_index_and_pairs_of_equal_magnitude():
    maps, cand = S.selection_case(3, 13, 21, 150, 7, mode="equal")
    key, pts = _select(maps, cand, 37, 37, None)
    assert bool((key[0] == 0).all()) and torch.equal(pts[0], cand[0, :37])     # row 0: all equal
    _check_selection(maps, cand, 37, 37, None, separated=False)
    maps, cand = S.selection_case(3, 13, 22, 150, 8, mode="pairs")
    cand[0, 75:, 0] = (cand[0, :75, 0] + 0.5) % 1.0          # mirrored partners: -v at the same offset
    cand[0, 75:, 1] = cand[0, :75, 1]
    _check_selection(maps, cand, 37, 50, torch.rand(3, 13, 2), separated=False)


def test_selection_production_row():
    g = torch.Generator().manual_seed(31)
    maps = torch.randn(1, 200, 334, generator=g) * 3.0
    cand = torch.rand(1, 37632, 2, generator=g)
    tail = torch.rand(1, 3136, 2, generator=g)
    _check_selection(maps, cand, 9408, 12544, tail, separated=False)


# ------------------------------------------------------------------------------ point loss
def _point_case(M, Np, L, seed, mode):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, Np, generator=g) * 3.0
    t = torch.rand(M, Np, generator=g).round() * torch.rand(M, Np, generator=g)
    if mode == "zeros":
        t.zero_()
    if mode == "ones":
        t.fill_(1.0)
    if mode == "big":
        x = torch.where(torch.rand(M, Np, generator=g) > 0.5, 100.0, -100.0)
    valid = torch.ones(M, dtype=torch.bool)
    if mode == "holes" and M > 1:
        valid[1] = False
    return x, t, valid


@pytest.mark.parametrize("M,L", [(1, 1), (3, 3), (40, 2)])
@pytest.mark.parametrize("Np", [1, 50, 12544])
@pytest.mark.parametrize("mode", ["random", "zeros", "ones", "big", "holes"])
def test_mask_point_loss_and_coefficients(M, L, Np, mode):
    hip = _hip()
    x, t, valid = _point_case(M, Np, L, M * 100 + Np, mode)
    ntm = 2.5 if mode == "ones" else None
    Ml = M // L
    matched = torch.zeros(M, 4, dtype=torch.int64)
    matched[:, 0] = torch.arange(M) // Ml                    # (layer, -, -, -): rows in layer order
    matched[~valid] = -1
    sums, out = torch.empty(M, 4, device=DEV), torch.full((4 * L,), float("nan"), device=DEV)
    coef = torch.full((M, Np), float("nan"), device=DEV)
    hip.mask_point_loss(_dev(x), _dev(t), _dev(matched), L, 5.0, 3.0, 1.0, sums, out, coef,
                        num_total_masks=ntm or 0.0)
    r = S.mask_point_loss(x, t, valid, L, 5.0, 3.0, 1.0, ntm)
    r32 = S.mask_point_loss(x, t, valid, L, 5.0, 3.0, 1.0, ntm, torch.float32)
    K = math.ceil(Np / 256) + 10
    out = out.cpu()
    _ratio("k_mask_point_loss mask", out[:L], r["mask"], r["mask_mag"],
           K + 4 + Ml + 4 + _allow(r32["mask"], r["mask"], r["mask_mag"]))
    _ratio("k_mask_point_loss dice", out[L:2 * L], r["dice"], r["dice_mag"],
           2 * K + 10 + Ml + 4 + _allow(r32["dice"], r["dice"], r["dice_mag"]))
    assert torch.equal(out[2 * L:3 * L], r32["den"][:, 0]) and torch.equal(out[3 * L:], r32["den"][:, 1])
    c64, cmag = S.mask_point_coef(x, t, valid, L, 5.0, 3.0, 1.0, ntm)
    c32, _ = S.mask_point_coef(x, t, valid, L, 5.0, 3.0, 1.0, ntm, torch.float32)
    _ratio("k_mask_point_coef", coef, c64, cmag, 4 * K + 34 + _allow(c32, c64, cmag))
    assert float(coef.cpu()[~valid].abs().max() if (~valid).any() else 0.0) == 0.0
    assert _hip().lib().pn_mask_point_loss_f32(1 << 20, 1 << 20, 1 << 20, 0, Np, L, 0, 1.0, 1.0, 1.0, 0.0,
                                               1 << 20, 1 << 20, None, None) == -1     # M = 0: refused


# ------------------------------------------------------------------------------ scatter
@pytest.mark.parametrize("h,w,Np,M", [(2, 2, 12544, 1), (13, 21, 50, 3), (200, 334, 12544, 2),
                                      (13, 21, 257, 2)])
def test_point_scatter_grad(h, w, Np, M):
    hip = _hip()
    g = torch.Generator().manual_seed(h + w + Np)
    pts = torch.rand(M, Np, 2, generator=g)
    below1 = float(np.nextafter(np.float32(1), np.float32(0)))
    border = torch.tensor([(0.0, 0.0), (below1, below1), (1.0, 1.0), (0.0, 1.0), (0.5, 0.0),
                           (below1, 0.5)])[:min(6, Np)]
    pts[:, :border.shape[0]] = border
    if Np == 257:                       # importance sampling clusters: many points on one pixel
        pts[1] = 0.5 + (pts[1] - 0.5) * 0.05
    coef = torch.randn(M, Np, generator=g) * 1e-3
    grad = [torch.full((M, h, w), float("nan"), device=DEV) for _ in range(2)]
    scratch = torch.empty(hip.point_scatter_scratch_ints(M, Np, h, w), dtype=torch.int32, device=DEV)
    for gr in grad:
        scratch.fill_(-7)               # (the kernel initialises what it reads)
        hip.point_scatter_grad(_dev(coef), _dev(pts), gr, scratch)
    assert torch.equal(grad[0], grad[1])                         # bitwise on two launches
    ref, mag, cnt, coord = S.scatter(coef, pts, h, w)
    err = (grad[0].cpu().double() - ref).abs()
    r_mag = float((err / (U * mag + FLT_MIN)).max())
    r_all = float((err / ((cnt + 19) * U * mag + S.COORD * U * coord + FLT_MIN)).max())
    WORST["k_point_scatter_grad vs mag alone"] = max(WORST.get("k_point_scatter_grad vs mag alone", 0.0), r_mag)
    print("k_point_scatter_grad %dx%d Np %d: worst ratio %.3f against mag alone, %.4f of its bound"
          % (h, w, Np, r_mag, r_all))
    assert bool(torch.isfinite(grad[0]).all())
    assert bool((err <= (cnt + 15 + 4) * U * mag + S.COORD * U * coord + FLT_MIN).all()), (r_mag, r_all)
    assert float(grad[0].cpu()[cnt == 0].abs().max() if (cnt == 0).any() else 0.0) == 0.0
    if (h, w) == (2, 2):
        assert float(cnt.min()) > 1000


# ------------------------------------------------------------------------------ loss_cls
@pytest.mark.parametrize("rows", [8, 200, 4096])
@pytest.mark.parametrize("C", [2, 6, 134])
@pytest.mark.parametrize("L", [1, 9])
def test_ce_avg_and_grad(rows, C, L):
    hip = _hip()
    g = torch.Generator().manual_seed(rows + C + L)
    x = torch.randn(L, rows, C, generator=g) * 3.0
    y = torch.randint(0, C, (L, rows), generator=g)
    y[0] = C - 1                                                 # a layer with every row background
    cw = torch.tensor([1.0] * (C - 1) + [0.1])
    out = torch.full((L,), float("nan"), device=DEV)
    grad = torch.full((L, rows, C), float("nan"), device=DEV)
    hip.ce_avg(_dev(x), _dev(y), _dev(cw), out, 2.0)
    hip.ce_avg_grad(_dev(x), _dev(y), _dev(cw), grad, 2.0)
    v64, mag = S.ce_avg(x, y, cw, 2.0)
    v32, _ = S.ce_avg(x, y, cw, 2.0, torch.float32)
    chain = math.ceil(C / 64) + 2 * rows + 14 + math.ceil(math.log(C) + 1)
    _ratio("k_ce_avg", out, v64, mag, chain + _allow(v32, v64, mag))
    g64, gmag = S.ce_avg_grad(x, y, cw, 2.0)
    g32, _ = S.ce_avg_grad(x, y, cw, 2.0, torch.float32)
    z = (x.double().amax(-1, keepdim=True) - x.double()).clamp(max=88.0)
    _ratio("k_ce_avg_grad", grad, g64, gmag, rows + math.ceil(C / 64) + 14 + z + _allow(g32, g64, gmag))


# ------------------------------------------------------------------------------ the whole loss
def _loss_obj(case, **kw):
    from pairnet_amd import Mask2FormerLoss
    Q = case["cls"].shape[2]
    tc = dict(num_points=case["num_points"], oversample_ratio=3.0, importance_sample_ratio=0.75,
              mask_assigner=dict(type="MaskHungarianAssigner",
                                 cls_cost=dict(type="ClassificationCost", weight=2.0),
                                 mask_cost=dict(type="CrossEntropyLossCost", weight=5.0, use_sigmoid=True),
                                 dice_cost=dict(type="DiceCost", weight=5.0, pred_act=True, eps=1.0)),
              sampler=dict(type="MaskPseudoSampler"))
    return Mask2FormerLoss(case["num_classes"], Q, train_cfg=tc,
                           loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=2.0,
                                         reduction="mean", class_weight=case["class_weight"]), **kw)


def _run(case, points=None, obj=None, debug=True, **kw):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    obj = obj or _loss_obj(case)
    grads = {}
    out = obj.loss(_dev(case["cls"]), _dev(case["mask"]), case["gt_labels"], case["gt_masks"],
                   [dict()] * case["cls"].shape[1], grads=grads,
                   points=case["points"] if points is None else points, debug=debug, **kw)
    torch.cuda.synchronize()
    return obj, out, grads


def _propagated(case, r, coefficients=True):
    """First-order effect of the samples' own error (18 roundings of their mag) on every output,
    from float64 autograd through the statement: -> ({name: bound}, g_mask bound [M][h][w])."""
    L = case["cls"].shape[0]
    h, w = case["mask"].shape[-2:]
    M = r["matched"].shape[0]
    if M == 0:
        return {k: 0.0 for k in r["losses"]}, torch.zeros(0, h, w, dtype=torch.float64)
    hg, wg = next(m for m in case["gt_masks"] if m.shape[0]).shape[-2:]
    maps = case["mask"].reshape(-1, h, w)
    gt_all = torch.cat([m for m in case["gt_masks"] if m.shape[0]])
    dx = S.sample_err(maps, r["mask_rows"], r["pts"])
    dt = S.sample_err(gt_all, r["matched"][:, 3], r["pts"])
    valid = torch.ones(M, dtype=torch.bool)
    cfg = S.CFG
    names, per = {}, {}
    x = r["x"].clone().requires_grad_(True)
    t = r["t"].clone().requires_grad_(True)
    res = S.mask_point_loss(x, t, valid, L, cfg["w_mask"], cfg["w_dice"], cfg["dice_eps"])
    for key, pre in (("mask", "loss_mask"), ("dice", "loss_dice")):
        for l in range(L):
            gx, gt = torch.autograd.grad(res[key][l], (x, t), retain_graph=True)
            names[(pre if l == L - 1 else "d%d.%s" % (l, pre))] = float((gx.abs() * dx).sum() + (gt.abs() * dt).sum())
    for k in r["losses"]:
        names.setdefault(k, 0.0)
    if not coefficients:
        return names, None
    # coefficients: |J| applied to the errors, mask by mask (the dice part couples a mask's points)
    Ml = M // L
    den = res["den"].detach()
    dcoef = torch.zeros_like(r["x"])
    for m in range(M):
        dm, dd = den[m // Ml, 0], den[m // Ml, 1]

        def f(xm, tm):
            s = torch.sigmoid(xm)
            num, dn = 2.0 * (s * tm).sum() + cfg["dice_eps"], s.sum() + tm.sum() + cfg["dice_eps"]
            return cfg["w_mask"] * (s - tm) / dm + (cfg["w_dice"] / dd) * ((num - 2.0 * tm * dn) / (dn * dn)) * s * (1 - s)
        jx, jt = torch.autograd.functional.jacobian(f, (r["x"][m], r["t"][m]))
        dcoef[m] = jx.abs() @ dx[m] + jt.abs() @ dt[m]
    return names, S.scatter(dcoef, r["pts"], h, w)[0]       # (dcoef >= 0: the weighted sum itself)


def _check_whole(name, case, obj, out, grads, r, r32, ref32=None):
    L, B, Q, C1 = case["cls"].shape
    h, w = case["mask"].shape[-2:]
    Np = case["num_points"]
    M = r["matched"].shape[0]
    Ml = M // L
    K = math.ceil(Np / 256) + 10
    assert int(obj.assign_status.cpu()) == 0 and obj.last_on_device
    assert torch.equal(obj.last["matched"].cpu(), r["matched"])        # the planted assignments
    assert torch.equal(obj.last["labels"].cpu(), r["labels"])
    assert torch.equal(grads["mask_rows"].cpu(), r["mask_rows"])
    assert set(out) == set(r["losses"]) and all(v.dim() == 0 and v.is_cuda for v in out.values())
    prop, g_prop = _propagated(case, r)
    chain = dict(loss_cls=math.ceil(C1 / 64) + 2 * B * Q + 14 + math.ceil(math.log(C1) + 1),
                 loss_mask=K + 4 + Ml + 4, loss_dice=2 * K + 10 + Ml + 4)
    for k in sorted(out):
        base = k.split(".")[-1]
        ref, mag = float(r["losses"][k]), float(r["mags"][k])
        a = _allow(r32["losses"][k], ref, mag)
        err = abs(float(out[k]) - ref)
        bound = (chain[base] + a) * U * mag + prop[k] + FLT_MIN
        print("%s %s: ratio %.3f, bound %.3f roundings" % (name, k, err / (U * mag + FLT_MIN),
                                                           bound / (U * mag + FLT_MIN)))
        assert err <= bound, (name, k, err, bound)
        if ref32 is not None:      # against the reference's own fp32 value: c plus its stored ratio
            i = list(ref32["names"]).index(k)
            assert abs(float(out[k]) - float(ref32["loss32"][i])) <= \
                bound + float(ref32["loss_ratio"][i]) * U * mag, (name, k)
    z = (case["cls"].double().amax(-1, keepdim=True) - case["cls"].double()).clamp(max=88.0)
    _ratio(name + " g_cls", grads["cls"], r["g_cls"], r["g_cls_mag"],
           B * Q + math.ceil(C1 / 64) + 14 + z + _allow(r32["g_cls"], r["g_cls"], r["g_cls_mag"]))
    if ref32 is not None:
        err = (grads["cls"].cpu().double() - torch.from_numpy(ref32["g_cls32"]).double()).abs()
        c = B * Q + math.ceil(C1 / 64) + 14 + z + 4 + 2 * float(ref32["g_cls_ratio"])
        assert bool((err <= c * U * r["g_cls_mag"] + FLT_MIN).all())
    assert tuple(grads["mask"].shape) == (M, h, w)
    if M:
        cnt = S.scatter(torch.ones(M, r["pts"].shape[1]), r["pts"], h, w)[2]
        a = _allow(r32["g_mask"], r["g_mask"], r["g_mask_mag"] + S.COORD * r["g_mask_coord"])
        err = (grads["mask"].cpu().double() - r["g_mask"]).abs()
        bound = (4 * K + 34 + cnt + 15 + a) * U * r["g_mask_mag"] + S.COORD * U * r["g_mask_coord"] \
            + g_prop + FLT_MIN
        ratio = float((err / (U * r["g_mask_mag"] + FLT_MIN)).max())
        WORST[name + " g_mask"] = ratio
        print("%s g_mask: worst ratio %.3f against mag alone, %.4f of its bound"
              % (name, ratio, float((err / bound).max())))
        assert bool((err <= bound).all()), (name, ratio)
        if ref32 is not None:
            err = (grads["mask"].cpu().double() - torch.from_numpy(ref32["g_mask32"]).double()).abs()
            assert bool((err <= bound + float(ref32["g_mask_ratio"]) * U
                         * (r["g_mask_mag"] + S.COORD * r["g_mask_coord"])).all())


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("form", ["candidates", "loss"])
def test_whole_loss_on_the_fixture(name, form):
    case, ref32 = S.golden_case(name)
    pts = case["points"]
    if form == "loss":
        Ml = ref32["matched"].shape[0] // case["cls"].shape[0]
        lp = S.run_whole(case)["pts"]        # (the float64 statement's final loss points)
        pts = dict(assign=pts["assign"], loss=[lp[l * Ml:(l + 1) * Ml] for l in range(case["cls"].shape[0])])
    obj, out, grads = _run(case, pts)
    r, r32 = S.run_whole(case), S.run_whole(case, torch.float32)
    assert np.array_equal(r["matched"].numpy(), ref32["matched"])
    if form == "candidates":
        assert torch.equal(obj.last["points"].cpu(), r["pts"])
    _check_whole("fixture %s/%s" % (name, form), case, obj, out, grads, r, r32, ref32)


@pytest.mark.parametrize("name", ["l9", "g_gt_q"])
def test_whole_loss_on_drawn_cases(name):
    case = S.loss_case(**S.WHOLE_CASES[name])
    obj, out, grads = _run(case)
    r, r32 = S.run_whole(case), S.run_whole(case, torch.float32)
    for key, pairs in case["planted"].items():
        rows = r["matched"][(r["matched"][:, 0] == key[0]) & (r["matched"][:, 1] == key[1])]
        assert [int(q) for q in rows[:, 2]] == [q for q, _ in pairs]
    assert name != "l9" or len(case["planted"]) == 18            # 18 problems in ONE launch
    _check_whole(name, case, obj, out, grads, r, r32)


def test_whole_loss_without_any_ground_truth():
    case = S.loss_case(**S.WHOLE_CASES["empty"])
    obj, out, grads = _run(case)
    r, r32 = S.run_whole(case), S.run_whole(case, torch.float32)
    for k, v in out.items():
        if "cls" not in k:
            assert float(v) == 0.0, k
    assert tuple(grads["mask"].shape) == (0, 13, 21) and grads["mask_rows"].numel() == 0
    assert all(math.isfinite(float(v)) and float(v) > 0 for k, v in out.items() if "cls" in k)
    _check_whole("empty", case, obj, out, grads, r, r32)


def test_nan_in_one_mask_logit_sets_the_status_and_leaves_the_other_layers_alone():
    case = S.loss_case(**S.WHOLE_CASES["l9"])
    obj, clean, _ = _run(case)
    bad = dict(case, mask=case["mask"].clone())
    px, py = case["points"]["assign"][4][1][0].tolist()       # a pixel the first assign point reads
    bad["mask"][4, 1, 3, min(12, max(0, math.floor(py * 13 - 0.5) + 1)),
                min(20, max(0, math.floor(px * 21 - 0.5) + 1))] = float("nan")
    obj2, out, grads = _run(bad)
    assert int(obj2.assign_status.cpu()) != 0
    lab = obj2.last["labels"].cpu().view(9, 2, 8)
    assert bool((lab[4, 1] == case["num_classes"]).all())                 # targets at their fills
    m = obj2.last["matched"].cpu()
    Ml = m.shape[0] // 9
    assert bool((m[4 * Ml + 3:5 * Ml] == -1).all()) and bool((m[4 * Ml:4 * Ml + 3, 0] == 4).all())
    assert bool((grads["mask_rows"].cpu()[4 * Ml + 3:5 * Ml] == -1).all())
    for k in clean:
        if not k.startswith("d4."):
            assert torch.equal(out[k], clean[k]), k
        assert math.isfinite(float(out[k])), k


def test_same_seed_and_step_give_the_same_bits_and_another_step_other_points():
    case = S.loss_case(**S.WHOLE_CASES["g_gt_q"])
    none = dict()
    obj, o1, g1 = _run(case, none, seed=5, step=3)
    p1 = obj.last["points"].clone()
    _, o2, g2 = _run(case, none, obj=obj, seed=5, step=3)
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    assert all(torch.equal(g1[k], g2[k]) for k in g1) and torch.equal(p1, obj.last["points"])
    _, o3, _ = _run(case, none, obj=obj, seed=5, step=4)
    assert not torch.equal(p1, obj.last["points"])
    # the drawn points are the host Philox's: layer 1's candidates at site 4 * 1 + 1
    Ml, Sn = p1.shape[0] // 2, 150
    want = S.uniform(Ml * Sn * 2, 5, 0, 5, 4)
    assert np.array_equal(obj.last["candidates"].cpu().numpy()[Ml:].reshape(-1), want)


def test_production_shape_scalars():
    """L 9, B 2, Q 100, 200 x 334, Np 12 544, G = (23, 17): the shape labnotes R15 times; scalars only."""
    case = S.loss_case(9, 2, 100, 133, 200, 334, 12544, (23, 17), 41)
    obj, out, _ = _run(case, dict(), seed=1, step=1)
    assert int(obj.assign_status.cpu()) == 0
    pts = dict(assign=[[obj.last["assign"][(l, b)].cpu() for b in range(2)] for l in range(9)],
               loss=[obj.last["points"].cpu()[l * 40:(l + 1) * 40] for l in range(9)])
    r = S.run_whole(case, points=pts, grad=False)
    assert torch.equal(obj.last["matched"].cpu(), r["matched"])
    prop, _ = _propagated(case, r, coefficients=False)
    K, Ml = math.ceil(12544 / 256) + 10, 40
    chain = dict(loss_cls=3 + 400 + 14 + 6, loss_mask=K + 4 + Ml + 4, loss_dice=2 * K + 10 + Ml + 4)
    for k in sorted(out):
        ref, mag = float(r["losses"][k]), float(r["mags"][k])
        ratio = abs(float(out[k]) - ref) / (U * mag + FLT_MIN)
        WORST["production " + k.split(".")[-1]] = max(WORST.get("production " + k.split(".")[-1], 0.0), ratio)
        print("production %s: ratio %.3f" % (k, ratio))
        # (a = 4: the fp32 oracle run of this shape is not worth its minutes)
        assert abs(float(out[k]) - ref) <= (chain[k.split(".")[-1]] + 4) * U * mag + prop[k] + FLT_MIN, k


# ------------------------------------------------------------------------------ interface
def test_baseline_head_seg_losses_equal_the_loss_object_bitwise():
    from helpers import baseline_cfg, golden, oracle_baseline_head, overrides_of
    from oracle import seeded
    from pairnet_amd import CrossHeadBaseline, Mask2FormerLoss
    fx = golden("baseline_small")
    _, sd, _ = oracle_baseline_head(int(fx["weight_seed"]), overrides_of(fx))
    H, W, bs = int(fx["height"]), int(fx["width"]), int(fx["batch"])
    feats = seeded.seeded_feats(int(fx["feat_seed"]), bs, H, W)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[2.0] * 4)] * bs
    head = CrossHeadBaseline(**baseline_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    head.return_all_layers = True
    cls, masks = head.forward([f.to(DEV) for f in feats], metas)
    L, B, Q, h, w = masks["mask"].shape
    g = torch.Generator().manual_seed(3)
    gt_labels = [torch.randint(0, 133, (3,), generator=g) for _ in range(bs)]
    gt_masks = [(torch.rand(3, 2 * h, 2 * w, generator=g) > 0.5).to(torch.uint8) for _ in range(bs)]
    g1, g2 = {}, {}
    got = head.seg_losses(cls, masks, gt_labels, gt_masks, metas, grads=g1, seed=2, step=9)
    want = Mask2FormerLoss(head.num_classes, Q).loss(cls["cls"], masks["mask"], gt_labels, gt_masks,
                                                     metas, grads=g2, seed=2, step=9)
    assert len(got) == 3 * L and L == 9
    for k in want:
        assert torch.equal(got[k], want[k]) and math.isfinite(float(got[k])), k
    assert all(torch.equal(g1[k], g2[k]) for k in g2)
    assert int(head._seg_loss.assign_status.cpu()) == 0


def test_detector_val_seg_losses_and_the_siblings_full_loss_stays_refused():
    from helpers import baseline_cfg
    from pairnet_amd import CrossHeadBaseline, HalfSizeMasks, PSGTr
    from pairnet_amd.backbone import ResNet50Hip
    H, W = 96, 128
    head = CrossHeadBaseline(**baseline_cfg())
    head.init_weights(seed=3)
    det = PSGTr.from_parts(ResNet50Hip(depth=50), head).to(DEV)
    g = torch.Generator().manual_seed(11)
    img = torch.randn(2, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(90, 120, 3), scale_factor=[2.0] * 4, batch_input_shape=(H, W))] * 2
    gt_labels = [torch.tensor([3, 17, 90]), torch.tensor([5, 60])]
    raw = [(torch.rand(3, 90, 120, generator=g) > 0.6).numpy().astype(np.uint8),
           (torch.rand(2, 90, 120, generator=g) > 0.5).numpy().astype(np.uint8)]
    a = det.val_seg_losses(img, metas, gt_labels, raw, seed=4, step=2)
    half = [HalfSizeMasks(m, (H, W)) for m in det._prepare_gt_masks(img, raw)]
    b = det.val_seg_losses(img, metas, gt_labels, half, seed=4, step=2)
    assert len(a) == 27 and head.return_all_layers is False
    for k in a:
        assert torch.equal(a[k], b[k]) and math.isfinite(float(a[k])), k
    with pytest.raises(NotImplementedError):                     # the siblings' full loss stays refused
        det.val_losses(img, metas, None, None, gt_labels, raw)
    with pytest.raises(NotImplementedError):
        det.trainer()


def test_crosshead2_detector_val_losses_is_bitwise_the_loss_object_run_directly():
    """No existing path changes: a `CrossHead2` detector's `val_losses` is, bit for bit, `CrossHead2Loss`
    run directly on the head's outputs and the prepared masks; it has no segmentation losses."""
    from helpers import head_cfg
    from pairnet_amd import CrossHead2, PSGTr
    from pairnet_amd.backbone import ResNet50Hip
    from pairnet_amd.losses import CrossHead2Loss
    H, W = 96, 128
    head = CrossHead2(**head_cfg())
    head.init_weights(seed=3)
    det = PSGTr.from_parts(ResNet50Hip(depth=50), head).to(DEV)
    g = torch.Generator().manual_seed(11)
    img = torch.randn(2, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(90, 120, 3), scale_factor=[2.0] * 4, batch_input_shape=(H, W))] * 2
    gt_labels = [torch.tensor([3, 17, 90, 120, 3]), torch.tensor([5, 60, 7])]
    raw = [(torch.rand(5, 90, 120, generator=g) > 0.6).numpy().astype(np.uint8),
           (torch.rand(3, 90, 120, generator=g) > 0.5).numpy().astype(np.uint8)]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 3, 17], [1, 0, 56], [4, 2, 5]]),
               torch.tensor([[0, 1, 2], [2, 1, 30]])]
    pts = [torch.rand(1, 12544, 2, generator=g) for _ in range(2)]
    got = det.val_losses(img, metas, gt_rels, None, gt_labels, raw, point_coords=pts)
    got = {k: v.clone() for k, v in got.items()}
    cls, masks = head.forward(det.extract_feat(img), metas)
    cfg = head_cfg()
    direct = CrossHead2Loss(head.num_classes, head.num_relations, head.num_obj_query, head.num_rel_query,
                            train_cfg=cfg.get("train_cfg"), rel_cls_loss=cfg.get("rel_cls_loss"),
                            subobj_cls_loss=cfg.get("subobj_cls_loss"),
                            importance_match_loss=cfg.get("importance_match_loss"))
    want = direct.loss(cls, masks, gt_rels, None, gt_labels, det._prepare_gt_masks(img, raw), metas,
                       point_coords=pts)
    assert set(got) == {"loss_r_cls", "loss_sub_cls", "loss_obj_cls", "loss_match"}
    for k in want:
        assert torch.equal(got[k], want[k]) and math.isfinite(float(got[k])), k
    with pytest.raises(NotImplementedError):
        det.val_seg_losses(img, metas, gt_labels, raw)
