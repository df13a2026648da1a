"""GPU: every forward / value kernel of csrc/loss.hip (k_ce_mean, k_seesaw_mean, k_bce_posw_mean,
k_mask_match_cost, k_id_match_cost, k_point_sample) and every kernel of csrc/optim.hip
(k_sumsq_partial + k_clip_coef, k_adamw plain and guarded), one at a time against the float64
statements of tests/loss_optim_ref.py (pinned to the oracle / torch functions without a GPU by
tests/test_loss_optim_refs.py), at the smallest shapes that reach each branch.  The backward
kernels beside them are bounded in tests/test_grad_kernels_gpu.py.

Bounds.  |got - ref| <= c 2^-24 mag + FLT_MIN on every output element, `mag` the float64
computation on absolute values.  c = L + a is never taken from the kernel under test:
  L  the longest chain of fp32 roundings an output passes through, counted from the kernel's
     source and written as a formula of the shape beside each test;
  a  the allowance for the device math functions (expf, logf, log1pf, powf, division): twice the
     ratio the same oracle function reaches when torch evaluates it in fp32 on the same inputs
     (against its own float64 run, with the same mag), and at least 4.
Every case prints the kernel's ratio, the fp32 oracle's ratio and c; the worst of each per kernel
is printed when the module ends (labnotes/r14.md records them).  The optimizer's bounds are
derived alone (the norm is a double sum: 2^-23 relative; AdamW: rounding counts of k_adamw's
expression plus 2).  Integer and data-movement results, untouched outputs and refused calls are
compared bitwise; kernels that claim a fixed order are launched twice and must agree bitwise."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

import loss_optim_ref as R
from test_grad_kernels_gpu import FLT_MIN, U, _gen, _randn, _within, _within_rows  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
WORST = {}          # kernel -> (kernel ratio, fp32-oracle ratio, c, case)


@pytest.fixture(scope="module")
def hip(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip as h
    h.lib()
    yield h
    print("\n%-18s %12s %14s %8s  case" % ("kernel", "worst ratio", "fp32 oracle", "c"))
    for k, (r, o, c, case) in sorted(WORST.items()):
        print("%-18s %12.3f %14.3f %8g  %s" % (k, r, o, c, case))


def _ratio(got, ref, mag):
    err = (got.detach().to(DEV).double() - ref).abs()
    ratio = (err - FLT_MIN).clamp_min(0.0) / (U * mag)
    ratio = torch.where(err <= FLT_MIN, torch.zeros_like(ratio), ratio)
    return float(ratio.max())


def _note(kernel, case, worst, oracle, c):
    if kernel not in WORST or worst > WORST[kernel][0]:
        WORST[kernel] = (worst, oracle, c, case)


def _bounded(kernel, case, got, ref, mag, L, o32):
    """c = L + max(4, 2 x the fp32 oracle's ratio); asserts the bound on every element.  L may be
    a tensor (a count per element); the printed c is then the largest."""
    ref = ref.detach().to(DEV).double().reshape(got.shape)
    mag = mag.detach().to(DEV).double().expand(got.shape) if mag.dim() == 0 else \
        mag.detach().to(DEV).double().reshape(got.shape)
    oracle = _ratio(o32.reshape(got.shape), ref, mag)
    a = max(4.0, 2.0 * oracle) if math.isfinite(oracle) else 4.0
    c = L + a
    if torch.is_tensor(c):
        c, mag = float(c.max()), mag * (c / c.max())
        L = float(L.max())
    print("%-60s fp32 oracle %8.3f  L %g  c %g" % (kernel + " " + case, oracle, L, c))
    worst = _within(kernel + " " + case, got, ref, mag, c)
    _note(kernel, case, worst, oracle, c)
    return worst


def _exp_arg(logits, labels):
    """The roundings a softmax entry inherits from its exponent: x - m is rounded once (2^-24
    |x - m|) and exp() turns that absolute error into a relative one, so the entry carries
    |x[label] - max x| roundings; beyond 88 the entry is below FLT_MIN, which the additive term
    covers.  Per element [rows][labels], from the inputs alone."""
    x = logits.double()
    return (x.amax(-1, keepdim=True) - x[:, labels]).clamp(max=88.0)


def _targets(g, rows, C, ignore):
    t = torch.randint(0, C, (rows,), generator=g, device=DEV)
    if ignore == "some":
        t[::3] = -1
    elif ignore == "all":
        t[:] = -1
    return t


def _strided(x, extra):
    """x as a column slice of a tensor `extra` columns wider, NaN beyond the slice."""
    if not extra:
        return x
    wide = torch.full((x.shape[0], x.shape[1] + extra), NAN, device=DEV)
    wide[:, :x.shape[1]] = x
    return wide[:, :x.shape[1]]


# ============================================================ ce_mean
# (rows, C, extra ld, ignore, class weights, big): every rows and C of the issue's list; rows =
# 3 / 4 / 5 straddle the four waves, C = 63 / 64 / 65 the lane stride, 4096 = LOSS_MAX_ROWS
CE_CASES = [(1, 1, 0, "none", False, False), (1, 134, 7, "none", True, True),
            (3, 2, 0, "some", False, True), (4, 63, 7, "none", True, True),
            (5, 64, 0, "some", True, False), (5, 65, 7, "none", False, True),
            (200, 134, 0, "some", True, True), (200, 134, 7, "all", True, False),
            (200, 2, 7, "none", False, False), (4096, 134, 0, "some", False, True),
            (4096, 1, 7, "none", True, False), (4096, 65, 0, "all", False, False),
            (4096, 63, 7, "some", True, True)]


@pytest.mark.parametrize("rows,C,extra,ignore,weighted,big", CE_CASES)
def test_ce_mean(hip, rows, C, extra, ignore, weighted, big):
    from oracle import mmdet_train as T
    lw = 2.0
    g = _gen(rows * 7 + C + extra + weighted * 3 + big * 13 + len(ignore))
    x = _randn(g, rows, C, scale=3.0)
    t = _targets(g, rows, C, ignore)
    if big and C >= 8:                                       # logits at +-80 (test_ce_mean_grad)
        x[::2, 5] = 80.0
        x[1::4, :] = -80.0
        x[1::4, 7] = 80.0
    if big and C >= 2 and ignore != "all":     # a target at -80 under a +80 competitor: loss 160
        r = min(1, rows - 1)
        t[r] = 0
        x[r, 0], x[r, C - 1] = -80.0, 80.0
    x = _strided(x, extra)
    cw = (torch.rand(C, generator=g, device=DEV) + 0.5) if weighted else None
    out = torch.full((2,), NAN, device=DEV)
    out2 = torch.full((2,), NAN, device=DEV)
    hip.ce_mean(x, t, cw, out[0:1], lw)
    hip.ce_mean(x, t, cw, out2[0:1], lw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[1])), "wrote past its one output"
    assert torch.equal(out[0:1], out2[0:1]), "ce_mean is not bitwise reproducible"
    kept = t >= 0
    if not bool(kept.any()):
        assert float(out[0]) == 0.0 and not math.copysign(1.0, float(out[0])) < 0
        return
    ref, mag = R.ce_mean(x, t, cw, lw)
    o32 = lw * T.cross_entropy(x[kept], t[kept], class_weight=cw)
    # L: x - m 1 (carried by exp() into the sum: at most ln C + 1 relative to it), lane sum
    # ceil(C / 64), wave sum 6, + m 1, - x[y] 1, cw 1, serial row sum `rows`, / n 1, lw 1
    L = math.ceil(C / 64) + rows + 12 + math.ceil(math.log(C) + 1.0)
    _bounded("ce_mean", "rows %d C %d ld+%d ignore %s cw %d big %d" % (
        rows, C, extra, ignore, weighted, big), out[0:1], ref, mag, L, o32)


# ============================================================ seesaw_mean
def _seesaw_cases():
    rows_of, out = [1, 5, 200, 4096], []
    for i, (C, pq, kind) in enumerate(itertools.product([2, 57, 64], [(0.8, 2.0), (0.0, 2.0),
                                                                        (0.8, 0.0), (0.0, 0.0)],
                                                        ["zeros", "spread"])):
        ignore = "all" if i % 8 == 5 else ("some" if i % 2 == 0 else "none")
        out.append((C, pq[0], pq[1], kind, rows_of[(i + i // 4) % 4], 7 * (i % 3 == 1), ignore))
    return out


@pytest.mark.parametrize("C,p,q,cum_kind,rows,extra,ignore", _seesaw_cases())
def test_seesaw_mean(hip, C, p, q, cum_kind, rows, extra, ignore):
    from oracle import mmdet_train as T
    lw, eps = 1.0, 1e-2
    g = _gen(rows + C + int(p * 10) + int(q * 100) + len(cum_kind) + extra)
    x = _randn(g, rows, C, scale=2.0)
    t = _targets(g, rows, C, ignore)
    if cum_kind == "zeros":
        cum = torch.randint(0, 50, (C,), generator=g, device=DEV).float()
        cum[:min(8, C)] = 0.0                       # (clamped to 1 by the reference)
        if ignore != "all":
            t[::7] = torch.arange(rows, device=DEV)[::7] % min(8, C)
    else:
        cum = torch.pow(10.0, torch.rand(C, generator=g, device=DEV) * 5.0).round()
    if ignore != "all":                              # a row whose target score is far below eps
        r = min(4, rows - 1)
        t[r] = 1
        x[r] = 5.0
        x[r, 1] = -10.0
    x = _strided(x, extra)
    out = torch.full((2,), NAN, device=DEV)
    out2 = torch.full((2,), NAN, device=DEV)
    hip.seesaw_mean(x, t, cum, out[0:1], p, q, eps, lw)
    hip.seesaw_mean(x, t, cum, out2[0:1], p, q, eps, lw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[1])) and torch.equal(out[0:1], out2[0:1])
    kept = t >= 0
    if not bool(kept.any()):
        assert float(out[0]) == 0.0
        return
    ref, mag = R.seesaw_mean(x, t, cum, p, q, eps, lw)
    o32 = lw * T.seesaw_ce_loss(x[kept], t[kept], None, cum, C, p, q, eps)
    # L: softmax x - m 1, wave sum 6, / 1, score ratio / 1 = 9, doubled by powf(., q <= 2) = 18;
    # w *= 2, x + log w 1, x' - m2 1, wave sum 6, + m2 1, - x[y] 1, serial row sum `rows`, / n 1,
    # lw 1
    L = rows + 32
    _bounded("seesaw_mean", "C %d p %g q %g cum %s rows %d ld+%d ignore %s" % (
        C, p, q, cum_kind, rows, extra, ignore), out[0:1], ref, mag, L, o32)


# ============================================================ bce_posw_mean
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2 * 100 * 100, 2 * 200 * 200])
@pytest.mark.parametrize("pos", ["one", "all", "random"])
def test_bce_posw_mean(hip, n, pos):
    lw = 5.0
    big = (n + len(pos)) % 2 == 0 or n >= 20000
    g = _gen(n + len(pos))
    x = _randn(g, n, scale=3.0)
    if big:                                               # logits at +-100
        x[::3] = 100.0
        x[1::3] = -100.0
    t = torch.zeros(n, device=DEV)
    if pos == "one":
        t[n // 2] = 1.0
    elif pos == "all":
        t[:] = 1.0
    else:
        t = (torch.rand(n, generator=g, device=DEV) < 0.05).float()
        t[0] = 1.0
    out = torch.full((3,), NAN, device=DEV)
    out2 = torch.full((3,), NAN, device=DEV)
    hip.bce_posw_mean(x, t, out[0:2], lw)
    hip.bce_posw_mean(x, t, out2[0:2], lw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[2])) and torch.equal(out[0:2], out2[0:2])
    ref, mag, pw32 = R.bce_posw_mean(x, t, lw)
    assert np.float32(float(out[1])) == pw32, (float(out[1]), pw32)
    o32 = lw * F.binary_cross_entropy_with_logits(x, t, pos_weight=out[1].clone())
    # L: element: pw 1, pw - 1 1, * t 1, 1 + 1, (1 - t) x 2, softplus + 1, * 1, + 1 = 9; strided
    # sum ceil(n / 1024), wave sum 6, 16 waves; / n 1, lw 1
    L = math.ceil(n / 1024) + 6 + 16 + 11
    _bounded("bce_posw_mean", "n %d pos %s big %d" % (n, pos, big), out[0:1], ref, mag, L, o32)


# ============================================================ mask_match_cost
# (Q, G, Np, ncls, (w_cls, w_mask, w_dice), seed): every Q, G, Np and ncls of the issue's list;
# the two seeded cases with the config's weights are the assignment cases (tests/
# test_loss_optim_refs.py checks their planted margin without a GPU on the same numbers)
MASK_CASES = [(1, 1, 1, 2, (2.0, 5.0, 5.0), 1), (1, 7, 255, 134, (0.0, 5.0, 0.0), 2),
              (100, 8, 256, 134, (2.0, 0.0, 0.0), 3), (1, 9, 257, 300, (0.0, 0.0, 5.0), 4),
              (100, 16, 257, 300, (2.0, 5.0, 5.0), 5), (1, 17, 255, 2, (2.0, 5.0, 5.0), 6),
              (100, 7, 256, 2, (0.0, 0.0, 5.0), 7), (100, 1, 12544, 134, (0.0, 5.0, 0.0), 8),
              (100, 9, 12544, 134, (2.0, 5.0, 5.0), 41), (100, 17, 12544, 134, (2.0, 5.0, 5.0), 42),
              (100, 17, 12544, 300, (2.0, 0.0, 0.0), 9)]


@pytest.mark.parametrize("Q,G,Np,ncls,w,seed", MASK_CASES)
def test_mask_match_cost(hip, Q, G, Np, ncls, w, seed):
    from oracle import mmdet_train as T
    cls, labels, x, t, planted = (v.to(DEV) if torch.is_tensor(v) else v
                                  for v in R.mask_cost_case(Q, G, Np, ncls, seed))
    cost = torch.full((Q * G + 1,), NAN, device=DEV)
    hip.mask_match_cost(cls, labels, x, t, cost[:Q * G].view(Q, G), w[0], w[1], w[2], 1.0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(cost[-1])), "wrote past the Q x G matrix"
    got = cost[:Q * G].view(Q, G)
    ref, mag = R.mask_match_cost(cls, labels, x, t, w[0], w[1], w[2], 1.0)
    o32 = T.ClassificationCost(w[0])(cls, labels) + T.CrossEntropyLossCost(w[1])(x, t) + \
        T.DiceCost(w[2], pred_act=True, eps=1.0)(x, t)
    # K = ceil(Np / 256) + 6 + 4 is a strided block sum (lane chain, wave sum, 4 waves).
    #   class:  x - m 1, block sum of ncls, entry: - 1 and _exp_arg, / 1, w 1
    #   mask:   softplus + 1 (or x t 1), K, s_neg - a 1, / Np 1, w 1
    #   dice:   numerator sigmoid 2, s t 1, K, + eps 1; denominator sigmoid 2, K, + c 1, + eps 1:
    #           the quotient carries both, / 1, 1 - 1, w 1
    # the terms present (weight != 0) add; two more roundings join them
    K = math.ceil(Np / 256) + 10
    terms = [math.ceil(ncls / 256) + 10 + 4 + _exp_arg(cls, labels), K + 4.0 + 0.0 * ref,
             2 * K + 11.0 + 0.0 * ref]
    L = torch.stack([Lt for Lt, wt in zip(terms, w) if wt != 0.0]).amax(0) + 2
    _bounded("mask_match_cost", "Q %d G %d Np %d ncls %d w %s" % (Q, G, Np, ncls, w), got, ref,
             mag, L, o32)
    if planted and w == (2.0, 5.0, 5.0) and Np == 12544:
        r64, c64 = linear_sum_assignment(ref.cpu().numpy())
        r32, c32 = linear_sum_assignment(got.cpu().numpy())
        assert float(R.assignment_margin(ref, r64, c64).min()) > 1e-3
        assert np.array_equal(r64, r32) and np.array_equal(c64, c32)
        assert dict(zip(r32.tolist(), c32.tolist())) == planted


# ============================================================ id_match_cost
ID_CASES = [(1, 1, 56, (1.0, 1.0, 0.5)), (100, 63, 57, (1.0, 1.0, 0.5)),
            (200, 64, 56, (1.0, 0.0, 0.0)), (100, 65, 57, (0.0, 1.0, 0.0)),
            (200, 130, 56, (0.0, 0.0, 0.5)), (1, 130, 57, (1.0, 1.0, 0.5))]


@pytest.mark.parametrize("Rq,G,nrel,w", ID_CASES)
def test_id_match_cost(hip, Rq, G, nrel, w):
    from oracle import mmdet_train as T
    ncls = 134
    g = _gen(Rq * 3 + G + nrel)
    sub, obj, rel = (_randn(g, Rq, n, scale=3.0) for n in (ncls, ncls, nrel))
    sub[0, 3], obj[0, 4], rel[0, nrel - 1] = 80.0, -80.0, 80.0
    sub[Rq - 1, ::2] = -80.0
    gs, go, gr = (torch.randint(0, n, (G,), generator=g, device=DEV) for n in (ncls, ncls, nrel))
    gs[0], go[0], gr[0] = 3, 4, nrel - 1
    gs[-1], gr[-1] = ncls - 1, 0
    cost = torch.full((Rq * G + 1,), NAN, device=DEV)
    hip.id_match_cost(sub, obj, rel, gs, go, gr, cost[:Rq * G].view(Rq, G), w[0], w[1], w[2])
    torch.cuda.synchronize()
    assert bool(torch.isnan(cost[-1]))
    ref, mag = R.id_match_cost(sub, obj, rel, gs, go, gr, w[0], w[1], w[2])
    o32 = T.ClassificationCost(w[0])(sub, gs) + T.ClassificationCost(w[1])(obj, go) + \
        T.ClassificationCost(w[2])(rel, gr)
    # L: x - m 1, lane sum ceil(134 / 64), wave sum 6, entry - 1 and _exp_arg, / 1, w 1, two
    # additions
    Z = torch.stack([_exp_arg(a, b) for a, b, wt in ((sub, gs, w[0]), (obj, go, w[1]),
                                                     (rel, gr, w[2])) if wt != 0.0]).amax(0)
    L = math.ceil(ncls / 64) + 6 + 4 + 2 + Z
    _bounded("id_match_cost", "R %d G %d nrel %d w %s" % (Rq, G, nrel, w),
             cost[:Rq * G].view(Rq, G), ref, mag, L, o32)


# ============================================================ point_sample
def _points(g, h, w, Np):
    """Np points: the corners (exactly 0 and 1), points far outside (-5, 7), pixel centres
    (j + 0.5) / w, points in [-0.1, 1.1] and random points in [0, 1]; -> pts, slice of the far
    points, slice of the centres (Np = 1: one centre)."""
    corners = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0]], device=DEV)
    far = torch.tensor([[-5.0, 0.5], [0.5, 7.0], [7.0, -5.0], [-5.0, -5.0]], device=DEV)
    k = max(1, min(h * w, Np // 4))
    pix = torch.randperm(h * w, generator=g, device=DEV)[:k]
    # pixel ((o - 1) / 2 of each axis, o the odd part of its length): its centre 2^-(a + 1) is a
    # binary fraction, the one kind of centre an fp32 coordinate can hit exactly
    odd = lambda v: v // (v & -v)
    pix[0] = ((odd(h) - 1) // 2) * w + (odd(w) - 1) // 2
    centres = torch.stack([((pix % w).float() + 0.5) / w, ((pix // w).float() + 0.5) / h], 1)
    wide = torch.rand(max(Np // 4, 1), 2, generator=g, device=DEV) * 1.2 - 0.1
    rnd = torch.rand(Np, 2, generator=g, device=DEV)
    if Np == 1:
        return centres[:1].contiguous(), slice(0, 0), slice(0, 1)
    pts = torch.cat([corners, far, centres, wide, rnd])[:Np].contiguous()
    return pts, slice(4, min(8, Np)), slice(min(8, Np), min(8 + k, Np))


@pytest.mark.parametrize("kind", ["float", "u8", "bool"])
@pytest.mark.parametrize("h,w,Np", [(1, 1, 1), (1, 7, 255), (9, 1, 256), (25, 42, 257),
                                    (200, 334, 12544), (25, 42, 12544), (1, 7, 1)])
def test_point_sample(hip, kind, h, w, Np):
    from oracle import mmdet_train as T
    P = 3
    g = _gen(h * 1000 + w + Np + len(kind))
    if kind == "float":
        maps = _randn(g, P, h, w)
    else:
        maps = torch.rand(P, h, w, generator=g, device=DEV) > 0.5
        maps = maps.to(torch.uint8) if kind == "u8" else maps
    pts, far, centres = _points(g, h, w, Np)
    out = torch.full((P * Np + 1,), NAN, device=DEV)
    hip.point_sample(maps, pts, out[:P * Np].view(P, Np))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[-1])), "wrote past the P x Np samples"
    got = out[:P * Np].view(P, Np)
    ref, top = R.point_sample(maps, pts)
    o32 = T.point_sample(maps.float().unsqueeze(1), pts.unsqueeze(0).repeat(P, 1, 1)).squeeze(1)
    # mag = (1 + max(h, w)) max |tap|: the fp32 pixel coordinate ((c + 1) w - 1) / 2 carries
    # 2^-24 w of error and the sample moves by that times the local difference.
    # L: coordinates x and y: + 1, * w, - 1 each = 6; weights: two differences 2, product 1; tap
    # * weight 1; four additions
    mag = ((1.0 + max(h, w)) * top)[:, None].expand(P, Np)
    _bounded("point_sample", "%s %dx%d Np %d" % (kind, h, w, Np), got, ref, mag, 14, o32)
    assert bool((got[:, far] == 0).all()), "a point far outside must sample exact zeros"
    if kind != "float":
        # at a pixel centre the sample is the pixel.  Exactly so where the fp32 coordinate lands
        # on the centre exactly (((c + 1) w - 1) / 2 an integer in exact arithmetic: then every
        # fp32 operation of the chain is exact, fused or not); elsewhere to within the
        # coordinate's rounding, which the bound above states
        c = R.point_grid(pts[centres]).double()
        ix, iy = ((c[:, 0] + 1.0) * w - 1.0) / 2.0, ((c[:, 1] + 1.0) * h - 1.0) / 2.0
        exact = (ix == ix.round()) & (iy == iy.round())
        assert bool(exact.any())
        v = got[:, centres][:, exact]
        assert bool(((v == 0) | (v == 1)).all())
        assert torch.equal(v.double(), ref[:, centres][:, exact])


# ============================================================ grad_norm_clip
def _grads(g, n, kind):
    if kind == "normal":
        return _randn(g, n, scale=0.01)
    if kind == "zero":
        return torch.zeros(n, device=DEV)
    if kind == "tiny":                       # squares underflow fp32
        return torch.full((n,), 1e-30, device=DEV)
    if kind == "huge":                       # squares overflow fp32
        return torch.full((n,), 1e25, device=DEV)
    x = torch.full((n,), 1e-6, device=DEV)   # "spike"
    x[n // 2] = 1e4
    return x


# n = 4096 p + r: 1 .. 256 partial sums (the chunk is ceil(n / parts)); 256 * 4096 + 1 is the
# first n whose chunk exceeds 4096
NORM_CASES = [(1, 1.0, "normal", 0.1), (255, 0.5, "normal", 0.1), (4095, 0.125, "normal", 0.0),
              (4096, 1.0, "zero", 0.1), (4097, 1.0, "tiny", 0.1), (4097, 1.0, "huge", 0.1),
              (4097, 0.5, "normal", 0.1), (5184, 0.5, "spike", 0.1), (5184, 1.0, "normal", -1.0),
              (256 * 4096, 1.0, "normal", 0.1), (256 * 4096 + 1, 0.5, "spike", 0.1),
              (256 * 4096 + 1, 0.125, "normal", 0.1), (3000001, 0.125, "normal", 0.1),
              (3000001, 1.0, "tiny", 0.1), (3000001, 0.5, "zero", 0.0), (1, 1.0, "huge", 0.1)]


@pytest.mark.parametrize("n,pre,kind,max_norm", NORM_CASES)
def test_grad_norm_clip(hip, n, pre, kind, max_norm):
    g = _gen(n + len(kind))
    x = _grads(g, n, kind)
    outs = []
    for _ in range(2):
        out = torch.full((3,), NAN, device=DEV)
        scratch = torch.full((257,), NAN, device=DEV, dtype=torch.float64)
        hip.grad_norm_clip(x, out[0:2], scratch[:256], pre=pre, max_norm=max_norm)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[2])) and bool(torch.isnan(scratch[256]))
        outs.append(out[0:2].clone())
    assert torch.equal(outs[0], outs[1]), "grad_norm_clip is not bitwise reproducible"
    norm, coef = R.grad_norm_clip(x, pre, max_norm)
    got = outs[0].double()
    name = "grad_norm_clip n %d pre %g %s max_norm %g" % (n, pre, kind, max_norm)
    if kind == "zero":
        assert float(got[0]) == 0.0
    if kind == "zero" or max_norm <= 0:
        assert float(got[1]) == 1.0
    # the double sum is exact to n 2^-53; sqrt and the rounding to fp32: 2^-23 relative.  The
    # coefficient: norm 2, + 1e-6 1, max_norm to fp32 and the division: 2^-22 relative
    ref = torch.tensor([norm], dtype=torch.float64, device=DEV)
    w0 = _within(name + " norm", got[0:1], ref, ref, 2.0)
    cref = torch.tensor([coef], dtype=torch.float64, device=DEV)
    w1 = _within(name + " coef", got[1:2], cref, cref, 4.0)
    _note("grad_norm_clip", name, max(w0, w1), 0.0, 4.0)


# ============================================================ adamw / adamw_guarded
def _adamw_state(g, nseg, gscale, zero_state):
    sizes, offs = R.segment_layout(nseg, seed=nseg)
    n = int(offs[-1])
    live = torch.zeros(n, dtype=torch.bool, device=DEV)
    seg = torch.zeros(n, dtype=torch.int64, device=DEV)
    for s in range(nseg):
        live[offs[s]:offs[s] + sizes[s]] = True
        seg[offs[s]:offs[s + 1]] = s
    rnd = lambda: torch.rand(n, generator=g, device=DEV)
    # |p| log-uniform over [1e-6, 1], exact zeros; gradients with exact zeros
    p = torch.pow(10.0, -6.0 * rnd()) * torch.where(rnd() < 0.5, -1.0, 1.0)
    p[rnd() < 0.05] = 0.0
    gr = _randn(g, n, scale=gscale)
    gr[rnd() < 0.05] = 0.0
    if zero_state:
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    else:
        m, v = _randn(g, n, scale=gscale), rnd() * gscale * gscale
        both = rnd() < 0.05                      # v = 0 with g = 0: the denominator is eps alone
        v[both], gr[both] = 0.0, 0.0
    for a in (p, gr, m, v):
        a[~live] = 0.0                           # padding, as train.py lays it out
    return sizes, offs, n, live, seg, p, gr, m, v


@pytest.mark.parametrize("nseg", [1, 3, 257])
@pytest.mark.parametrize("step", [1, 2, 3, 10, 1000, 100000])
def test_adamw(hip, nseg, step):
    b1, b2, eps = 0.9, 0.999, 1e-8
    k = [1, 2, 3, 10, 1000, 100000].index(step) + (nseg % 3)
    lr, wd = ((1e-4, 1e-4), (1e-3, 1e-2))[k % 2]
    use_clip, pre = (k // 2) % 2 == 0, (1.0, 0.5)[(k // 2 + k) % 2]
    gscale, zero_state = (1e-3, 10.0)[(k + nseg) % 2], step == 1 or (step == 10 and nseg == 3)
    g = _gen(nseg * 1000 + step)
    sizes, offs, n, live, seg, p0, gr, m0, v0 = _adamw_state(g, nseg, gscale, zero_state)
    lm, wm = ([1.0, 0.1, 1.0] * nseg)[:nseg], ([1.0, 1.0, 0.0] * nseg)[:nseg]
    lr_mult, wd_mult = torch.tensor(lm, device=DEV), torch.tensor(wm, device=DEV)
    seg_off = torch.from_numpy(offs).to(DEV)
    clip = torch.tensor([123.0, 0.37], device=DEV) if use_clip else None
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    hip.adamw(p, gr, m, v, seg_off, lr_mult, wd_mult, lr, b1, b2, eps, wd, step, clip=clip, pre=pre)
    # the guarded entry with guard 0 is the same update; with a non-zero guard nothing moves
    pg, mg, vg = p0.clone(), m0.clone(), v0.clone()
    hip.adamw(pg, gr, mg, vg, seg_off, lr_mult, wd_mult, lr, b1, b2, eps, wd, step, clip=clip,
              pre=pre, guard=torch.zeros(1, dtype=torch.int32, device=DEV))
    pat = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, device=DEV, dtype=torch.int64)
           .to(torch.int32) for _ in range(3)]
    held = [t.clone().view(torch.float32) for t in pat]
    hip.adamw(held[0], gr, held[1], held[2], seg_off, lr_mult, wd_mult, lr, b1, b2, eps, wd, step,
              clip=clip, pre=pre, guard=torch.tensor([-7], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    for a, b in zip(held, pat):
        assert torch.equal(a.view(torch.int32), b), "a non-zero guard must leave every byte"
    for a, b in ((p, pg), (m, mg), (v, vg)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "guard 0 != plain entry"
    for a in (p, m, v):                       # zero padding stays zero bit for bit
        assert bool((a[~live].view(torch.int32) == 0).all()), "padding moved"

    # the effective gradient is rounded in fp32 before the mathematics starts: (g pre) clip[1]
    gi = gr * R.f32(pre)
    if use_clip:
        gi = gi * clip[1]
    # a group's lr and weight decay as torch holds them: products of Python doubles
    lr_el = torch.tensor([lr * x for x in lm], dtype=torch.float64, device=DEV)[seg]
    wd_el = torch.tensor([wd * x for x in wm], dtype=torch.float64, device=DEV)[seg]
    p1, m1, v1, mag_m, mag_v, mag_d = R.adamw_step(p0, gi, m0, v0, lr_el, wd_el, b1, b2, eps, step)
    name = "adamw nseg %d step %d lr %g wd %g clip %d pre %g g %g zero %d" % (
        nseg, step, lr, wd, use_clip, pre, gscale, zero_state)
    # m = m + (g - m) c1: three roundings, + 2
    wm = _within(name + " m", m, m1, mag_m, 5.0)
    # v = b2 v + c2 g g: four roundings, + 2
    wv = _within(name + " v", v, v1, mag_v, 6.0)
    # p: the decay product and the final subtraction round p: 2 u |p|.  The update: step size 5
    # (lr, the multiplier and bc1 to fp32, their product, the division), m 3, the denominator 6
    # (v's 4 halved by the root 2, sqrt 1, / 1, eps to fp32 1, + 1), m / denom 1, * 1 = 16, + 2
    mag_p = 2.0 * p0.double().abs() + 18.0 * mag_d
    wp = _within(name + " p", p, p1, mag_p, 1.0)
    edge = torch.from_numpy(np.unique(np.concatenate([offs[1:] - 1, offs[:-1], [n - 1]]))).to(DEV)
    _within(name + " p at segment edges", p[edge], p1[edge], mag_p[edge], 1.0)
    _within(name + " v at segment edges", v[edge], v1[edge], mag_v[edge], 6.0)
    assert bool(live[torch.from_numpy(offs[:-1]).to(DEV)].all()) and bool(live[n - 1])
    _note("adamw m", name, wm, 0.0, 5.0)
    _note("adamw v", name, wv, 0.0, 6.0)
    _note("adamw p", name, wp, 0.0, 1.0)


# ============================================================ refusals
def test_value_kernels_refuse_what_they_cannot_run(hip):
    """The C ABI refuses (error code, nothing written) what its kernels cannot run."""
    z = lambda *s: torch.zeros(*s, device=DEV)
    zi = lambda *s: torch.zeros(*s, dtype=torch.int64, device=DEV)
    nan = lambda *s: torch.full(s, NAN, device=DEV)
    lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
    outs = []
    # rows = LOSS_MAX_ROWS + 1
    o = nan(2)
    with pytest.raises(RuntimeError):
        hip.ce_mean(z(4097, 3), zi(4097), None, o[0:1], 1.0)
    with pytest.raises(RuntimeError):
        hip.seesaw_mean(z(4097, 3), zi(4097), z(3), o[1:2], 0.8, 2.0, 1e-2, 1.0)
    outs.append(o)
    # seesaw: more classes than lanes
    o = nan(1)
    with pytest.raises(RuntimeError):
        hip.seesaw_mean(z(5, 65), zi(5), z(65), o, 0.8, 2.0, 1e-2, 1.0)
    outs.append(o)
    # a row stride below the row length
    o = nan(2)
    x = z(5, 8)
    assert lib.pn_ce_mean_f32(x.data_ptr(), 7, zi(5).data_ptr(), None, o.data_ptr(), 5, 8, 1.0,
                              st) != 0
    assert lib.pn_seesaw_mean_f32(x.data_ptr(), 7, zi(5).data_ptr(), z(8).data_ptr(),
                                  o[1:].data_ptr(), 5, 8, 0.8, 2.0, 1e-2, 1.0, st) != 0
    outs.append(o)
    # points at an address that is not a multiple of 8
    o = nan(2, 16)
    pts = z(33)[1:33].view(16, 2)
    assert pts.data_ptr() % 8 == 4
    with pytest.raises(RuntimeError):
        hip.point_sample(z(2, 4, 4), pts, o)
    outs.append(o)
    # n = 0
    o = nan(4)
    with pytest.raises(RuntimeError):
        hip.bce_posw_mean(z(0), z(0), o[0:2], 1.0)
    with pytest.raises(RuntimeError):
        hip.grad_norm_clip(z(0), o[2:4], torch.zeros(256, dtype=torch.float64, device=DEV))
    assert lib.pn_grad_norm_clip_f32(z(4).data_ptr(), 0, 1.0, 0.1, o[2:].data_ptr(),
                                     torch.zeros(256, dtype=torch.float64, device=DEV).data_ptr(),
                                     st) != 0
    outs.append(o)
    # AdamW: step 0, a beta >= 1, n = 0, a NULL guard on the guarded entry
    n = 64
    p, m, v = nan(n), nan(n), nan(n)
    so, sl, sw = torch.tensor([0, n], device=DEV), torch.ones(1, device=DEV), torch.ones(1, device=DEV)
    for b1, b2, step in ((0.9, 0.999, 0), (1.0, 0.999, 1), (0.9, 1.0, 1), (0.9, 1.5, 1),
                         (-0.1, 0.999, 1)):
        for guard in (None, torch.zeros(1, dtype=torch.int32, device=DEV)):
            with pytest.raises(RuntimeError):
                hip.adamw(p, z(n), m, v, so, sl, sw, 1e-3, b1, b2, 1e-8, 1e-2, step, guard=guard)
    args = [p.data_ptr(), z(n).data_ptr(), m.data_ptr(), v.data_ptr(), n, so.data_ptr(),
            sl.data_ptr(), sw.data_ptr(), 1, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, None, 1.0]
    assert lib.pn_adamw_guarded_f32(*args, None, st) != 0
    args[4] = 0
    assert lib.pn_adamw_f32(*args, st) != 0
    torch.cuda.synchronize()
    for t in outs + [p, m, v]:
        assert bool(torch.isnan(t).all()), "a refused call wrote to its output"
