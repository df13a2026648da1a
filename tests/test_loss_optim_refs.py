"""CPU: the float64 statements of tests/loss_optim_ref.py (the references of
tests/test_loss_optim_kernels_gpu.py) against the functions they restate -- the oracle's
cross_entropy / seesaw_ce_loss / match costs / point_sample, torch's BCE-with-logits and
grid_sample, torch.optim.AdamW with clip_grad_norm_ -- to 1e-12, and the planted margins of the
mask_match_cost assignment cases."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

import loss_optim_ref as R
from oracle import mmdet_train as T

TOL = 1e-12


def _close(got, want, scale=None):
    got = torch.as_tensor(got, dtype=torch.float64)
    want = torch.as_tensor(want, dtype=torch.float64)
    scale = want.abs().clamp(min=1.0) if scale is None else scale
    err = float(((got - want).abs() / scale).max())
    assert err <= TOL, err


def _targets(g, rows, C, ignore):
    t = torch.randint(0, C, (rows,), generator=g)
    if ignore == "some":
        t[::3] = -1
    elif ignore == "all":
        t[:] = -1
    return t


@pytest.mark.parametrize("rows,C", [(1, 1), (5, 2), (200, 134)])
@pytest.mark.parametrize("ignore", ["none", "some", "all"])
@pytest.mark.parametrize("weighted", [False, True])
def test_ce_mean_statement_is_the_oracle_cross_entropy(rows, C, ignore, weighted):
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g) * 3.0
    x[0, 0] = -80.0
    t = _targets(g, rows, C, ignore)
    cw = torch.rand(C, generator=g) + 0.5 if weighted else None
    val, mag = R.ce_mean(x, t, cw, 2.0)
    kept = t >= 0
    if not bool(kept.any()):
        assert float(val) == 0.0 and float(mag) == 0.0
        return
    want = 2.0 * T.cross_entropy(x.double()[kept], t[kept],
                                 class_weight=None if cw is None else cw.double())
    _close(val, want)
    assert float(mag) >= abs(float(val))


@pytest.mark.parametrize("C", [2, 57, 64])
@pytest.mark.parametrize("p,q", [(0.8, 2.0), (0.0, 2.0), (0.8, 0.0), (0.0, 0.0)])
@pytest.mark.parametrize("cum_kind", ["zeros", "spread"])
def test_seesaw_mean_statement_is_the_oracle_seesaw_ce_loss(C, p, q, cum_kind):
    rows, eps = 50, 1e-2
    g = torch.Generator().manual_seed(C + int(p * 10) + int(q * 100))
    x = torch.randn(rows, C, generator=g) * 2.0
    t = _targets(g, rows, C, "some")
    t[4] = 1
    x[4] = 5.0
    x[4, 1] = -10.0                                 # target score far below eps
    if cum_kind == "zeros":
        cum = torch.randint(0, 50, (C,), generator=g).float()
        cum[:2] = 0.0
    else:
        cum = torch.pow(10.0, torch.rand(C, generator=g) * 5.0).round()
    val, mag = R.seesaw_mean(x, t, cum, p, q, eps, 1.5)
    kept = t >= 0
    want = 1.5 * T.seesaw_ce_loss(x.double()[kept], t[kept], None, cum.double(), C, p, q, eps)
    _close(val, want)
    assert float(mag) >= abs(float(val))
    v0, m0 = R.seesaw_mean(x, torch.full_like(t, -1), cum, p, q, eps, 1.5)
    assert float(v0) == 0.0 and float(m0) == 0.0


@pytest.mark.parametrize("n", [1, 1025])
@pytest.mark.parametrize("pos", ["one", "all", "random"])
def test_bce_posw_mean_statement_is_torch_bce_with_logits(n, pos):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 3.0
    x[::3], x[1::3] = 100.0, -100.0
    t = torch.zeros(n)
    if pos == "one":
        t[n // 2] = 1.0
    elif pos == "all":
        t[:] = 1.0
    else:
        t = (torch.rand(n, generator=g) < 0.05).float()
        t[0] = 1.0
    val, mag, pw32 = R.bce_posw_mean(x, t, 5.0)
    pw = torch.tensor(float(n) / float(t.gt(0).sum()), dtype=torch.float64)
    want = 5.0 * F.binary_cross_entropy_with_logits(x.double(), t.double(), pos_weight=pw)
    _close(val, want)
    assert float(mag) >= abs(float(val)) and pw32.dtype == np.float32
    assert abs(float(pw32) - float(pw)) <= 2.0 ** -24 * float(pw)


# (Q, G, Np, ncls, weights): the GPU file's cases at small Np, and its two assignment cases
MASK_SMALL = [(1, 1, 1, 2, (2.0, 5.0, 5.0)), (3, 7, 255, 134, (0.0, 5.0, 0.0)),
              (4, 9, 257, 300, (2.0, 0.0, 0.0)), (5, 17, 256, 134, (0.0, 0.0, 5.0))]
ASSIGN_CASES = [(100, 9, 12544, 134, 41), (100, 17, 12544, 134, 42)]


@pytest.mark.parametrize("Q,G,Np,ncls,w", MASK_SMALL)
def test_mask_match_cost_statement_is_the_oracle_costs(Q, G, Np, ncls, w):
    cls, labels, x, t, _ = R.mask_cost_case(Q, G, Np, ncls, seed=Q + G + Np)
    assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    cost, mag = R.mask_match_cost(cls, labels, x, t, w[0], w[1], w[2], 1.0)
    want = T.ClassificationCost(w[0])(cls.double(), labels) + \
        T.CrossEntropyLossCost(w[1])(_Keep64(x), _Keep64(t)) + \
        T.DiceCost(w[2], pred_act=True, eps=1.0)(x.double(), _Keep64(t))
    _close(cost, want)
    assert bool((mag >= cost.abs() - 1e-12).all())


class _Keep64:
    """A float64 view that survives the oracle costs' `.float()` (they cast their inputs to
    fp32; the statement is checked against their formula in float64)."""

    def __init__(self, t):
        self.t = t.double()

    def flatten(self, d):
        return _Keep64(self.t.flatten(d))

    def float(self):
        return self.t


@pytest.mark.parametrize("Q,G,Np,ncls,seed", ASSIGN_CASES)
def test_assignment_cases_have_their_planted_margin(Q, G, Np, ncls, seed):
    cls, labels, x, t, planted = R.mask_cost_case(Q, G, Np, ncls, seed)
    assert bool((t[0] == 0).all()) and bool((t[-1] == 1).all())
    assert 0 in labels.tolist() and ncls - 2 in labels.tolist()
    assert float(x.max()) == 80.0 and bool((x[Q - 1] == -80.0).all())
    cost, _ = R.mask_match_cost(cls, labels, x, t, 2.0, 5.0, 5.0, 1.0)
    rows, cols = linear_sum_assignment(cost.numpy())
    assert dict(zip(rows.tolist(), cols.tolist())) == planted
    assert float(R.assignment_margin(cost, rows, cols).min()) > 1e-3


@pytest.mark.parametrize("R_,G,nrel", [(1, 1, 56), (7, 65, 57)])
def test_id_match_cost_statement_is_the_oracle_costs(R_, G, nrel):
    g = torch.Generator().manual_seed(R_ + G)
    sub, obj, rel = (torch.randn(R_, n, generator=g) * 3.0 for n in (134, 134, nrel))
    sub[0, 3], obj[0, 4] = 80.0, -80.0
    gs, go, gr = (torch.randint(0, n, (G,), generator=g) for n in (134, 134, nrel))
    cost, mag = R.id_match_cost(sub, obj, rel, gs, go, gr, 1.0, 1.0, 0.5)
    want = T.ClassificationCost(1.0)(sub.double(), gs) + T.ClassificationCost(1.0)(obj.double(), go) \
        + T.ClassificationCost(0.5)(rel.double(), gr)
    _close(cost, want)
    _close(mag, -want)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (9, 1), (25, 42)])
def test_point_sample_statement_is_grid_sample(h, w):
    g = torch.Generator().manual_seed(h * 50 + w)
    maps = torch.randn(3, h, w, generator=g)
    pts = torch.cat([torch.rand(300, 2, generator=g), torch.rand(200, 2, generator=g) * 1.2 - 0.1,
                     torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [-5.0, 0.5], [0.5, 7.0],
                                   [7.0, -5.0]]),
                     torch.stack([(torch.arange(w).float()[:1] + 0.5) / w,
                                  (torch.arange(h).float()[:1] + 0.5) / h], 1)])
    out, top = R.point_sample(maps, pts)
    grid = R.point_grid(pts).double()[None, :, None, :].expand(3, -1, -1, -1)
    want = F.grid_sample(maps.double()[:, None], grid, mode="bilinear", padding_mode="zeros",
                         align_corners=False)[:, 0, :, 0]
    _close(out, want)
    _close(top, maps.abs().amax((1, 2)))
    # the oracle's point_sample on the same fp32 points differs only by 2 p - 1 taken in fp32
    assert bool((out[:, -7:-1][:, 3:] == 0).all())           # far outside: no tap inside the map


def test_grad_norm_clip_statement_is_clip_grad_norm():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5184, generator=g) * 0.01
    for pre, max_norm in ((1.0, 0.1), (0.5, 0.1), (0.125, 0.0), (1.0, -1.0)):
        norm, coef = R.grad_norm_clip(x, pre, max_norm)
        p = torch.zeros(5184, dtype=torch.float64, requires_grad=True)
        p.grad = (x * np.float32(pre)).double()
        before = p.grad.clone()
        want = torch.nn.utils.clip_grad_norm_([p], max_norm if max_norm > 0 else float("inf"))
        _close(norm, want)
        _close(before * coef, p.grad, scale=before.abs().max())
    assert R.grad_norm_clip(torch.zeros(7), 1.0, 0.1) == (0.0, 1.0)
    n30, _ = R.grad_norm_clip(torch.full((4097,), 1e-30), 1.0, 0.1)
    assert abs(n30 - float(np.float32(1e-30)) * math.sqrt(4097)) < 1e-12 * n30
    n25, c25 = R.grad_norm_clip(torch.full((4097,), 1e25), 1.0, 0.1)
    assert math.isfinite(n25) and abs(c25 - 0.1 / n25) < 1e-12 * c25


@pytest.mark.parametrize("lr,wd", [(1e-4, 1e-4), (1e-3, 1e-2)])
def test_adamw_statement_is_three_steps_of_torch_adamw_with_clipping(lr, wd):
    """float64 parameters: the statement with double scalars equals torch.optim.AdamW +
    clip_grad_norm_ over three segments with the (1, 0.1, 1) / (1, 1, 0) multipliers."""
    g = torch.Generator().manual_seed(5)
    sizes, lr_mult, wd_mult = [1000, 37, 1], [1.0, 0.1, 1.0], [1.0, 1.0, 0.0]
    b1, b2, eps, max_norm, pre = 0.9, 0.999, 1e-8, 0.1, 0.5
    ref_p = [torch.randn(s, generator=g).double().requires_grad_() for s in sizes]
    opt = torch.optim.AdamW([dict(params=[p], lr=lr * lm, weight_decay=wd * wm)
                             for p, lm, wm in zip(ref_p, lr_mult, wd_mult)], betas=(b1, b2), eps=eps)
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ref_p]
    for step in range(1, 4):
        grads = [torch.randn(s, generator=g) * (10.0 if step == 2 else 0.001) for s in sizes]
        norm, coef = R.grad_norm_clip(torch.cat(grads), pre, max_norm)
        for p, gr in zip(ref_p, grads):
            p.grad = (gr * np.float32(pre)).double()
        want_norm = torch.nn.utils.clip_grad_norm_(ref_p, max_norm)
        _close(norm, want_norm)
        opt.step()
        for i, (gr, lm, wm) in enumerate(zip(grads, lr_mult, wd_mult)):
            p, m, v = mine[i]
            gi = (gr * np.float32(pre)).double() * coef
            p, m, v, _, _, _ = R.adamw_step(p, gi, m, v, lr * lm, wd * wm, b1, b2, eps, step,
                                            scalars=float)
            mine[i] = (p, m, v)
            st = opt.state[ref_p[i]]
            _close(p, ref_p[i].detach())
            _close(m, st["exp_avg"], scale=st["exp_avg"].abs().max())
            _close(v, st["exp_avg_sq"], scale=st["exp_avg_sq"].abs().max())


@pytest.mark.parametrize("step", [1, 2, 3, 10, 1000, 100000])
def test_adamw_statement_in_fp32_is_torch_adamw_on_fp32_parameters(step):
    """fp32 parameters: torch applies the four scalars rounded to fp32; the float64 statement
    with those scalars stays within a few fp32 roundings of torch's fp32 step, and differs from
    the double-scalar statement by the scalars' rounding (visible in v: 1 - beta2)."""
    lr, wd, b1, b2, eps = 1e-3, 1e-2, 0.9, 0.999, 1e-8
    g = torch.Generator().manual_seed(step)
    p0, gr = torch.randn(500, generator=g), torch.randn(500, generator=g) * 0.01
    m0, v0 = torch.randn(500, generator=g) * 0.01, torch.rand(500, generator=g) * 1e-4
    p = p0.clone().requires_grad_()
    opt = torch.optim.AdamW([p], lr=lr, weight_decay=wd, betas=(b1, b2), eps=eps, foreach=False)
    p.grad = gr.clone()
    opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=m0.clone(),
                        exp_avg_sq=v0.clone())
    opt.step()
    p1, m1, v1, mag_m, mag_v, mag_d = R.adamw_step(p0, gr, m0, v0, lr, wd, b1, b2, eps, step)
    u = 2.0 ** -24
    st = opt.state[p]
    assert bool(((st["exp_avg"].double() - m1).abs() <= 5 * u * mag_m).all())
    assert bool(((st["exp_avg_sq"].double() - v1).abs() <= 6 * u * mag_v).all())
    assert bool(((p.detach().double() - p1).abs() <= 2 * u * p0.abs().double() + 18 * u * mag_d)
                .all())
    # the scalars the statement rounds
    c1, c2, ss, bs = R.adamw_scalars(lr, b1, b2, step)
    assert (c1, c2) == (float(np.float32(0.1)), float(np.float32(0.001)))
    assert c2 != float(np.float32(1.0) - np.float32(0.999))        # what fp32 arithmetic gives
    assert abs(ss - lr / (1 - b1 ** step)) <= u * ss and abs(bs * bs - (1 - b2 ** step)) <= 3 * u


def test_fp32_decay_factor_equals_the_double_one():
    """The kernel forms 1 - (lr lm)(wd wm) in fp32 from fp32 factors; for every combination the
    GPU test uses this is the fp32 rounding of the double expression torch evaluates."""
    f = np.float32
    for lr in (1e-4, 1e-3):
        for wd in (1e-4, 1e-2):
            for lm in (1.0, 0.1):
                for wm in (1.0, 0.0):
                    got = f(1.0) - (f(lr) * f(lm)) * (f(wd) * f(wm))
                    assert got == f(1.0 - (lr * lm) * (wd * wm)), (lr, wd, lm, wm)


def test_segment_layouts():
    for nseg in (1, 3, 257):
        sizes, offs = R.segment_layout(nseg, seed=nseg)
        assert len(sizes) == nseg and len(offs) == nseg + 1 and 1 in sizes or nseg == 1
        assert bool((offs[1:] - offs[:-1] >= sizes).all())
        assert offs[-1] == offs[-2] + sizes[-1]                      # the last one ends at n
        if nseg > 1:
            assert bool(((offs[1:] - offs[:-1])[:-1] > sizes[:-1]).any())   # padding exists
