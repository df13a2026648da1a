"""GPU: the four kernels of csrc/det_loss.hip one at a time, and `DeformableDETRLoss`
(pair-net_amd/det_losses.py) on synthetic head outputs, against the float64 statements of
tests/det_loss_ref.py (pinned without a GPU by tests/test_det_loss_refs.py).

Bounds: the rule of tests/test_loss_optim_kernels_gpu.py -- |got - ref| <= c 2^-24 mag + FLT_MIN,
c = L + a; a = max(4, 2 x the ratio the same statement reaches when torch evaluates it in fp32 on
the same inputs against its own float64 run); L counted from the kernel's source:

k_det_match_cost   L = 14: pn_box_match_cost_f32's statements (tests/test_bbox_loss_gpu.py counts
                   them), magnitude `bbox_loss_ref.cost_terms`.
k_det_focal        element  expf 1, 1 + e 1, / 1 (q), q q 1, a . 1, . bce 1 = 6 (bce = max + log1pf(e)
                   is 3 deep and joins at the last product); magnitude the element itself (every
                   factor is positive).
                   gradient bce 3, gamma . 1, . omq 1, q + . 1, a q^2 . 1, scale . 1 = 8 (a q^2 is 5
                   deep, w / avg 1: both shorter).
                   term sum  6 + the lane's serial adds (16 elements, + 1 per term it meets: <= T)
                   + 9 (butterfly 6, waves 3) + second pass ceil(nwg / 256) + 9 + / avg 1 + w 1
                   = 42 + T + ceil(nwg / 256); magnitude w sum |element| / avg.
k_det_box_loss     the longest chain, as tests/test_bbox_loss_gpu.py counts the same expressions;
                   the magnitudes (det_loss_ref.box_pair_terms, class `M`) carry the conditioning:
                   sums add their operands' magnitudes, products multiply them, a quotient takes
                   x.mag y.mag / y^2, so a cancellation keeps the size of what was cancelled.
                   L1 per pair   gt / f 1, + 1 (/ 2 exact), pred - . 1, three adds 3 = 6.
                   1 - GIoU      gt / f 1, + 1, tcx -+ 0.5 tw 1, . f 1, side 1, area2 1,
                                 area1 + area2 1, - overlap 1 (union), enclose - union 1, / 1,
                                 iou - . 1, 1 - . 1 = 12.
                   gradient      union 8, union^2 1, overlap / . 1, 1 / enclose - . 1 (g_un),
                                 g_ov - g_un 1, . ih 1 (g_iw), the corner's two adds 2, . f 1,
                                 a1 + a2 1, si . 1, sb sign - . 1 = 19.
                   per term + ceil(M / 256) serial adds + 9 + / avg 1 + w 1.
k_det_results      box: 0.5 w exact, cx -+ . 1, . W 1, clamp exact, / scale 1 = 3, magnitude
                   (|cx| + 0.5 |w|) W / scale; score: expf 1, 1 + . 1, 1 / . 1 = 3.

Integer outputs, guard words behind every buffer and refused calls are compared exactly; the
kernels that claim a fixed order are launched twice and must agree bitwise.  The worst ratios are
printed when the module ends (labnotes/r36.md records them)."""
import math

import numpy as np
import pytest
import torch

import bbox_loss_ref as BR
import det_loss_ref as R
from test_grad_kernels_gpu import FLT_MIN, U  # noqa: F401
from test_loss_optim_kernels_gpu import _bounded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GUARD = 8
L_COST, L_FOCAL, L_FOCAL_GRAD = 14, 6, 8
L_L1, L_GIOU, L_BOX_GRAD = 6, 12, 19
L_RES = 3
WORST = {}


@pytest.fixture(scope="module")
def hip(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip as h
    h.lib()
    yield h
    for k, v in sorted(WORST.items()):
        print("%-28s worst ratio %9.3f  %s" % (k, v[0], v[1]))


def _note(k, worst, case):
    if k not in WORST or worst > WORST[k][0]:
        WORST[k] = (worst, case)


def _guarded(n, dtype=torch.float32, fill=NAN):
    """n elements followed by GUARD guard words -> (view of the n, the whole buffer)."""
    if dtype == torch.float32:
        buf = torch.full((n + GUARD,), fill, device=DEV)
    else:
        buf = torch.full((n + GUARD,), -77, device=DEV, dtype=dtype)
    return buf[:n], buf


def _guards_intact(buf, n):
    tail = buf[n:]
    return bool(torch.isnan(tail).all()) if buf.dtype == torch.float32 else bool((tail == -77).all())


# ================================================================== pn_det_focal_f32
def _focal_sum_L(T, nwg):
    return L_FOCAL + 36 + T + math.ceil(nwg / 256)


def _run_focal(hip, x, labels, term, avg, w_cls=2.0, alpha=0.25, gamma=2.0):
    rows, C = x.shape
    T = avg.numel()
    n_part = hip.det_focal_partials(rows, C, T)
    assert n_part == math.ceil(rows * C / 4096) * T
    outs = []
    for _ in range(2):
        grad, gbuf = _guarded(rows * C)
        part, pbuf = _guarded(n_part)
        out, obuf = _guarded(T)
        hip.det_focal(x, labels, term, avg, grad.view(rows, C), part, out, w_cls, alpha, gamma)
        torch.cuda.synchronize()
        assert _guards_intact(gbuf, rows * C) and _guards_intact(pbuf, n_part) \
            and _guards_intact(obuf, T), "wrote past a buffer"
        outs.append((grad.view(rows, C).clone(), out.clone()))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and \
        torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)), \
        "pn_det_focal_f32 is not bitwise reproducible"
    return outs[0]


def _check_focal(hip, case, x, labels, term, avg_list, w_cls=2.0, alpha=0.25, gamma=2.0):
    rows, C = x.shape
    T = len(avg_list)
    avg = torch.tensor(avg_list, dtype=torch.float32, device=DEV)
    grad, out = _run_focal(hip, x, labels, term, avg, w_cls, alpha, gamma)
    lab64, x64 = labels.long(), x.double()
    el = R.focal_elements(x64, lab64, alpha, gamma)
    el32 = R.focal_elements(x, lab64, alpha, gamma)
    scale = (w_cls / avg.double())[term.long()].view(-1, 1)
    gref = R.focal_grad(x64, lab64, alpha, gamma) * scale
    g32 = R.focal_grad(x, lab64, alpha, gamma) * (torch.tensor(w_cls, device=DEV) / avg)[
        term.long()].view(-1, 1)
    _note("k_det_focal grad", _bounded("k_det_focal grad", case, grad, gref, gref.abs(),
                                       L_FOCAL_GRAD, g32), case)
    nwg = math.ceil(rows * C / 4096)
    for t in range(T):
        sel = term == t
        ref = w_cls * el[sel].sum() / avg_list[t]
        o32 = w_cls * (el32[sel].sum() / avg[t])
        _note("k_det_focal sum", _bounded("k_det_focal sum", case + " term %d" % t, out[t:t + 1],
                                          ref.view(1), ref.abs().view(1), _focal_sum_L(T, nwg),
                                          o32.view(1)), case)
    return grad, out


def _focal_inputs(rows, C, seed, big=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(rows, C, generator=g, device=DEV) * 3.0
    if big:                                   # |logit| up to 20, on positives and negatives
        x.view(-1)[::7] = 20.0
        x.view(-1)[3::11] = -20.0
    labels = torch.randint(0, C + 1, (rows,), generator=g, device=DEV).to(torch.int32)
    labels[::3] = C                           # background-only rows
    return x, labels


@pytest.mark.parametrize("C", [150, 3, 1])
@pytest.mark.parametrize("rows", [1, 255, 257])
def test_focal_one_term(hip, rows, C):
    x, labels = _focal_inputs(rows, C, rows * 31 + C)
    if rows > 1:
        labels[1] = 0                          # a positive at a +20 / -20 logit
        x[1, 0] = 20.0
        labels[rows - 1] = C - 1
        x[rows - 1, C - 1] = -20.0
    term = torch.zeros(rows, dtype=torch.int32, device=DEV)
    _check_focal(hip, "rows %d C %d" % (rows, C), x, labels, term, [float(max(rows // 5, 1))])


def test_focal_terms_meet_inside_a_workgroup_and_a_term_without_positives(hip):
    # 3 terms over 700 rows x 7 classes = 4900 elements (2 workgroups): term 0 ends behind row 100
    # (element 707: inside a float4, 707 % 4 == 3) and term 1 behind row 399 (element 2800), both
    # inside workgroup 0; term 1 has no positives and the factor 1
    rows, C = 700, 7
    x, labels = _focal_inputs(rows, C, 5)
    term = torch.zeros(rows, dtype=torch.int32, device=DEV)
    term[101:400] = 1
    term[400:] = 2
    labels[101:400] = C
    grad, out = _check_focal(hip, "3 terms, 700 x 7", x, labels, term, [9.0, 1.0, 23.0])
    assert float(out[1]) > 0.0
    # other alpha / gamma (powf path) and weight
    _check_focal(hip, "3 terms, alpha .4 gamma 1.5", x, labels, term, [9.0, 1.0, 23.0], 1.0, 0.4, 1.5)
    # a row whose term is outside [0, T): no loss, zero gradient; the others unchanged
    term2 = term.clone()
    term2[50] = 7
    term2[51] = -1
    avg = torch.tensor([9.0, 1.0, 23.0], device=DEV)
    g2, o2 = _run_focal(hip, x, labels, term2, avg)
    assert bool((g2[50:52] == 0).all())
    keep = torch.ones(rows, dtype=torch.bool, device=DEV)
    keep[50:52] = False
    assert torch.equal(g2[keep], grad[keep]) and torch.equal(o2[1:], out[1:])
    assert float(o2[0]) < float(out[0])


def test_focal_bad_label_is_nan_not_a_fault_and_refusals(hip):
    rows, C = 9, 5
    x, labels = _focal_inputs(rows, C, 8, big=False)
    labels[4] = C + 1
    labels[6] = -3
    term = torch.zeros(rows, dtype=torch.int32, device=DEV)
    term[5:] = 1
    avg = torch.tensor([2.0, 3.0], device=DEV)
    grad, out = _run_focal(hip, x, labels, term, avg)
    assert bool(torch.isnan(grad[4]).all()) and bool(torch.isnan(grad[6]).all())
    ok = torch.ones(rows, dtype=torch.bool, device=DEV)
    ok[4] = ok[6] = False
    assert bool(torch.isfinite(grad[ok]).all()) and bool(torch.isnan(out).all())
    lib = hip.lib()
    P = hip._ptr
    g = torch.full((rows * C + GUARD,), NAN, device=DEV)
    part = torch.full((2 + GUARD,), NAN, device=DEV)
    o = torch.full((2 + GUARD,), NAN, device=DEV)
    i32 = torch.int32
    s = torch.cuda.current_stream().cuda_stream

    def raw(x_=x, lab=labels, tm=term, av=avg, g_=g, p_=part, plen=2, o_=o, r=rows, c=C, T=2):
        pt = lambda t, d=torch.float32: None if t is None else P(t, d)
        return lib.pn_det_focal_f32(pt(x_), pt(lab, i32), pt(tm, i32), pt(av), pt(g_), pt(p_), plen,
                                    pt(o_), r, c, T, 2.0, 0.25, 2.0, s)
    for kw in (dict(x_=None), dict(lab=None), dict(tm=None), dict(av=None), dict(g_=None),
               dict(p_=None), dict(o_=None), dict(r=0), dict(c=0), dict(c=257), dict(T=0),
               dict(T=17), dict(plen=1), dict(r=1 << 31), dict(x_=x.view(-1)[1:]),
               dict(g_=g[1:])):
        assert raw(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(g).all()) and bool(torch.isnan(part).all()) and bool(torch.isnan(o).all())
    assert hip.det_focal_partials(0, 5, 2) == 0 and hip.det_focal_partials(1 << 31, 1, 1) == 0


# ================================================================== pn_det_match_cost_f32
def _cost_problem(rows, G, nc, seed):
    cls, box, labels, boxes, shapes = BR_inputs(rows, (G,), nc, seed)
    return cls[0], box[0], labels[0], boxes[0], shapes[0]


def BR_inputs(Q, Gs, nc, seed):
    from test_bbox_loss_gpu import _cost_inputs
    return _cost_inputs(Q, Gs, nc, seed)


def test_match_cost_many_problems_one_launch(hip):
    nc = 150
    spec = [(2, 1, False), (100, 7, False), (1300, 7, False), (1300, 1, True), (100, 1, False),
            (2, 7, True)]
    probs = [_cost_problem(r, G, nc, 20 + i) for i, (r, G, _) in enumerate(spec)]
    NG = sum(p[2].numel() for p in probs)
    cls = torch.cat([p[0] for p in probs]).to(DEV)
    box = torch.cat([p[1] for p in probs]).to(DEV)
    # the labels, then zeros: a binarised problem points its label offset into the zeros
    gt_labels = torch.cat([p[2] for p in probs] + [torch.zeros(NG, dtype=torch.int64)]).to(DEV)
    gt_boxes = torch.cat([p[3] for p in probs]).to(DEV)
    factor = torch.tensor([[p[4][1], p[4][0]] * 2 for p in probs], dtype=torch.float32, device=DEV)
    tab, where, off, g_off, r_off = [], [], GUARD, 0, 0
    for (rows, G, binar), p in zip(spec, probs):
        tab += [off, rows, G, g_off + (NG if binar else 0), g_off, r_off]
        where.append((off, rows, G, r_off))
        off += rows * G + GUARD
        g_off += G
        r_off += rows
    tab = torch.tensor(tab, dtype=torch.int64, device=DEV).view(-1, 6)
    costs = []
    for _ in range(2):
        cost = torch.full((off,), NAN, device=DEV)
        hip.det_match_cost(cls, box, gt_labels, gt_boxes, factor, tab, cost,
                           max(r * g for _, r, g, _ in where), **BR.CFG)
        torch.cuda.synchronize()
        costs.append(cost)
    assert torch.equal(costs[0].view(torch.int32), costs[1].view(torch.int32))
    cost = costs[0]
    written = torch.zeros(off, dtype=torch.bool)
    for (o, rows, G, ro), (_, _, binar), p in zip(where, spec, probs):
        gl = torch.zeros_like(p[2]) if binar else p[2]
        f = torch.tensor([p[4][1], p[4][0]] * 2, dtype=torch.float32)
        got = cost[o:o + rows * G].view(rows, G)
        ref, mag = BR.cost_terms(p[0], p[1], gl, p[3], f)
        assert bool(((R.match_cost(p[0], p[1], gl, p[3], f) - ref).abs() <= 1e-13 * mag).all())
        o32, _ = BR.cost_terms(p[0], p[1], gl, p[3], f, dtype=torch.float32)
        case = "rows %d G %d%s" % (rows, G, " binarised" if binar else "")
        _note("k_det_match_cost", _bounded("k_det_match_cost", case, got, ref, mag, L_COST,
                                           o32.to(DEV)), case)
        written[o:o + rows * G] = True
        if 2 <= rows <= 1024:       # the old entry's block, bit for bit
            old = torch.full((rows * G,), NAN, device=DEV)
            hip.box_match_cost(p[0][None].to(DEV).contiguous(), p[1][None].to(DEV).contiguous(),
                               gl.to(DEV), p[3].to(DEV), f[None].to(DEV),
                               torch.tensor([[0, G, 0, 0]], dtype=torch.int64, device=DEV), old,
                               rows * G, **BR.CFG)
            torch.cuda.synchronize()
            assert torch.equal(old.view(torch.int32), got.reshape(-1).view(torch.int32)), case
    assert bool(torch.isnan(cost.cpu()[~written]).all()), "wrote outside its blocks"


def test_match_cost_refusals_leave_the_fences(hip):
    cls, box, labels, boxes, shape = _cost_problem(10, 3, 7, 31)
    cls, box, labels, boxes = cls.to(DEV), box.to(DEV), labels.to(DEV), boxes.to(DEV)
    factor = torch.tensor([[shape[1], shape[0]] * 2] * 2, dtype=torch.float32, device=DEV)
    fence = torch.full((64,), NAN, device=DEV)
    good = [30, 10, 3, 0, 0, 0]
    lib, P = hip.lib(), hip._ptr
    s = torch.cuda.current_stream().cuda_stream

    def raw(tab, cls_=cls, cost_=fence, rows_len=10, max_cells=30, Pn=2, nc=7):
        pt = lambda t, d=torch.float32: None if t is None else P(t, d)
        return lib.pn_det_match_cost_f32(pt(cls_), P(box), rows_len, P(labels, torch.int64), 3,
                                         P(boxes), 3, P(factor), pt(tab, torch.int64), pt(cost_),
                                         64, max_cells, Pn, nc, 2.0, 5.0, 2.0, 0.25, 2.0, 1e-12,
                                         1e-6, s)
    T2 = lambda row: torch.tensor([row, good], dtype=torch.int64, device=DEV)
    for kw in (dict(cls_=None), dict(cost_=None), dict(rows_len=0), dict(max_cells=0),
               dict(max_cells=65536 * 1024 + 1), dict(Pn=0), dict(Pn=65536), dict(nc=0),
               dict(nc=257)):
        assert raw(T2(good), **kw) == -1, kw
    assert raw(None) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(fence).all())
    # descriptors outside their buffers / ranges: that block is left alone, the other is written
    for row in ([0, 0, 3, 0, 0, 0], [0, 10, 0, 0, 0, 0], [40, 10, 3, 0, 0, 0], [0, 10, 3, 1, 0, 0],
                [0, 10, 3, 0, 1, 0], [0, 10, 3, 0, 0, 1], [-1, 10, 3, 0, 0, 0], [0, 65537, 1, 0, 0, 0],
                [0, 1, 1025, 0, 0, 0], [0, 10, 3, 0, 0, -1]):
        assert raw(T2(row)) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(fence[:30]).all()) and bool(torch.isnan(fence[60:]).all()), row
        assert bool(torch.isfinite(fence[30:60]).all()), row
        fence.fill_(NAN)
    bad = labels.clone()
    bad[1] = 7
    assert lib.pn_det_match_cost_f32(P(cls), P(box), 10, P(bad, torch.int64), 3, P(boxes), 3,
                                     P(factor), P(T2(good)[1:], torch.int64), P(fence), 64, 30, 1, 7,
                                     2.0, 5.0, 2.0, 0.25, 2.0, 1e-12, 1e-6, s) == 0
    torch.cuda.synchronize()
    blk = fence[30:60].view(10, 3)
    assert bool(torch.isnan(blk[:, 1]).all()) and bool(torch.isfinite(blk[:, [0, 2]]).all())


# ================================================================== pn_det_box_loss_f32
def _pairs_case(M, seed, rows=90, NG=40, F=3, T=2):
    """M matched pairs over `rows` predictions, NG ground-truth boxes, F factor rows, T terms;
    pairs 0 .. 2 planted: nested, disjoint, partially overlapping.  No corner ties."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.cat([torch.rand(rows, 2, generator=g) * 0.6 + 0.2,
                      torch.rand(rows, 2, generator=g) * 0.3 + 0.05], -1)
    factor = torch.tensor([[160.0, 112.0] * 2, [128.0, 128.0] * 2, [96.0, 144.0] * 2])[:F]
    c, s = torch.rand(NG, 2, generator=g) * 0.6 + 0.2, torch.rand(NG, 2, generator=g) * 0.3 + 0.05
    gtn = torch.cat([c - s / 2, c + s / 2], -1)
    prow = torch.randperm(rows, generator=g)[:M]
    pgt = torch.randint(0, NG, (M,), generator=g)
    pf = torch.randint(0, F, (M,), generator=g)
    planted = [([0.5, 0.5, 0.2, 0.2], [0.3, 0.3, 0.8, 0.8]),        # nested
               ([0.2, 0.2, 0.1, 0.1], [0.6, 0.6, 0.9, 0.9]),        # disjoint
               ([0.4, 0.4, 0.3, 0.3], [0.45, 0.5, 0.85, 0.9])]      # partial overlap
    for i, (p, q) in enumerate(planted[:M]):
        pred[prow[i]] = torch.tensor(p)
        gtn[i] = torch.tensor(q)
        pgt[i] = i
    gt = gtn.clone()
    split = M - M // 3 if T == 2 else M
    pterm = torch.zeros(M, dtype=torch.int64)
    pterm[split:] = 1
    # gt boxes are pixels of the pair's own factor row: scale per pair through a private copy
    gt_rows = torch.stack([gtn[pgt[i]] * factor[pf[i]] for i in range(M)]) if M else gt[:0]
    pairs = torch.stack([prow, torch.arange(M), pf, pterm], 1).to(torch.int32) if M else None
    term_off = torch.tensor([0, split, M][:T + 1] if T == 2 else [0, M], dtype=torch.int32)
    return pred, gt_rows, factor, pairs, term_off


@pytest.mark.parametrize("M", [0, 1, 65])
def test_box_loss_two_terms(hip, M):
    T, w_bbox, w_iou = 2, 5.0, 2.0
    pred, gt, factor, pairs, term_off = _pairs_case(M, 40 + M)
    rows = pred.shape[0]
    avg_list = [float(max(M - M // 3, 1)), 3.0]
    avg = torch.tensor(avg_list, device=DEV)
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    outs = []
    for _ in range(2):
        gflat, gbuf = _guarded(rows * 4, fill=NAN)
        gflat.zero_()
        out, obuf = _guarded(T * 2)
        hip.det_box_loss(d(pred), d(gt) if M else None, d(factor), d(pairs), d(term_off), avg,
                         gflat.view(rows, 4), out.view(T, 2), w_bbox, w_iou)
        torch.cuda.synchronize()
        assert _guards_intact(gbuf, rows * 4) and _guards_intact(obuf, T * 2)
        outs.append((gflat.view(rows, 4).clone(), out.view(T, 2).clone()))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and \
        torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    grad, out = outs[0]
    if M == 0:
        assert bool((out == 0).all()) and bool((grad == 0).all())
        return
    pr, pf, pt = pairs[:, 0].long(), pairs[:, 2].long(), pairs[:, 3].long()
    t64 = R.box_pair_terms(pred[pr].double(), gt.double(), factor[pf].double())
    # the fp32 oracle: the same statements through torch in fp32 (values), autograd (gradient)
    p32 = pred[pr].clone().requires_grad_(True)
    tgt32 = R.xyxy_to_cxcywh(gt / factor[pf])
    l1_32 = (p32 - tgt32).abs().sum(-1)
    gl_32 = 1 - R.giou_aligned(R.cxcywh_to_xyxy(p32) * factor[pf],
                               R.cxcywh_to_xyxy(tgt32) * factor[pf])
    a_pair = torch.tensor(avg_list)[pt]
    (g32,) = torch.autograd.grad((w_bbox * l1_32 / a_pair + w_iou * gl_32 / a_pair).sum(), p32)
    a64 = a_pair.double().view(-1, 1)
    gref = w_bbox / a64 * t64["d_l1"] + w_iou / a64 * t64["d_gl"].val
    gmag = w_bbox / a64 + w_iou / a64 * t64["d_gl"].mag
    case = "M %d" % M
    _note("k_det_box_loss grad", _bounded("k_det_box_loss grad", case, grad[pr.to(DEV)], gref, gmag,
                                          L_BOX_GRAD, g32.to(DEV)), case)
    hit = torch.zeros(rows, dtype=torch.bool)
    hit[pr] = True
    assert bool((grad.cpu()[~hit] == 0).all()), "an unmatched row's gradient was written"
    for t in range(T):
        sel = pt == t
        n = int(sel.sum())
        extra = math.ceil(max(n, 1) / 256) + 11
        for j, (key, w, L, v32) in enumerate((("l1", w_bbox, L_L1, l1_32), ("gl", w_iou, L_GIOU, gl_32))):
            ref = w * t64[key].val[sel].sum() / avg_list[t]
            mag = w * t64[key].mag[sel].sum() / avg_list[t]
            o32 = (w * (v32.detach()[sel].sum() / avg_list[t])).float()
            if n == 0:
                assert float(out[t, j]) == 0.0
                continue
            _note("k_det_box_loss " + key, _bounded(
                "k_det_box_loss " + key, case + " term %d" % t, out[t, j].view(1), ref.view(1),
                mag.view(1), L + extra, o32.view(1).to(DEV)), case)


def test_box_loss_refusals_and_bad_pairs(hip):
    pred, gt, factor, pairs, term_off = _pairs_case(5, 77, T=1)
    rows = pred.shape[0]
    d = lambda t: t.to(DEV).contiguous()
    pred, gt, factor, pairs, term_off = d(pred), d(gt), d(factor), d(pairs), d(term_off)
    avg = torch.tensor([5.0], device=DEV)
    grad = torch.zeros(rows, 4, device=DEV)
    out = torch.full((2 + GUARD,), NAN, device=DEV)
    lib, P = hip.lib(), hip._ptr
    s = torch.cuda.current_stream().cuda_stream
    i32 = torch.int32

    def raw(box=pred, gtb=gt, fac=factor, pr=pairs, to=term_off, av=avg, g=grad, o=out, M=5, T=1,
            rows_len=rows, nb=5, nf=3):
        pt = lambda t, dt=torch.float32: None if t is None else P(t, dt)
        return lib.pn_det_box_loss_f32(pt(box), rows_len, pt(gtb), nb, pt(fac), nf, pt(pr, i32),
                                       pt(to, i32), M, T, pt(av), pt(g), pt(o), 5.0, 2.0, 1e-6, s)
    for kw in (dict(box=None), dict(fac=None), dict(to=None), dict(av=None), dict(g=None),
               dict(o=None), dict(pr=None), dict(gtb=None), dict(M=-1), dict(T=0), dict(T=17),
               dict(rows_len=0), dict(nf=0), dict(nb=0), dict(rows_len=1 << 31)):
        assert raw(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((grad == 0).all())
    # a pair that points outside a buffer: NaN sums, no gradient for it, no fault
    for col, val in ((0, rows), (0, -1), (1, 5), (2, 3)):
        bad = pairs.clone()
        bad[2, col] = val
        grad.zero_()
        assert raw(pr=bad) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[:2]).all()) and bool(torch.isnan(out[2:]).all())
        assert int((grad.abs().sum(-1) > 0).sum()) == 4
        out.fill_(NAN)
    # a term range outside the pair list
    assert raw(to=torch.tensor([0, 6], dtype=i32, device=DEV)) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:2]).all())


# ================================================================== pn_det_results_f32
def _results_case(hip, B, Q, C, K, rescale, seed, ties=False):
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(B, Q, C, generator=g) * 2.0
    box = torch.cat([torch.rand(B, Q, 2, generator=g), torch.rand(B, Q, 2, generator=g) * 0.5], -1)
    if ties:                       # equal logits at the top: flat indices 1, 4 and 5 of image 0
        cls[0].view(-1)[[4, 1, 5]] = 9.0
    box[0, 0] = torch.tensor([0.95, 0.02, 0.4, 0.3])              # needs the clamp on both sides
    cls[0, 0, 0] = 11.0                                            # ... and is ranked first
    metas = [dict(img_shape=(112 + 16 * b, 160 - 13 * b, 3),
                  scale_factor=np.array([1.25, 0.8, 1.25, 0.8], np.float32) * (1 + b))
             for b in range(B)]
    meta = torch.tensor([[m["img_shape"][0], m["img_shape"][1]] + m["scale_factor"].tolist()
                         for m in metas], dtype=torch.float32, device=DEV)
    i64 = lambda: torch.full((B, K), -5, dtype=torch.int64, device=DEV)
    idx, qt, rm = i64(), i64(), i64()
    hip.topk_strided(cls.to(DEV), 1, Q * C, idx, qt, rm, B, Q * C, C, K)
    det, dbuf = _guarded(B * K * 5)
    labels, lbuf = _guarded(B * K, torch.int64)
    hip.det_results(cls.to(DEV), box.to(DEV), idx, meta, det.view(B, K, 5), labels.view(B, K), rescale)
    torch.cuda.synchronize()
    assert _guards_intact(dbuf, B * K * 5) and _guards_intact(lbuf, B * K)
    det, labels = det.view(B, K, 5), labels.view(B, K)
    case = "Q %d C %d K %d rescale %s" % (Q, C, K, rescale)
    for b in range(B):
        m = metas[b]
        ref, rl = R.get_bboxes_single(cls[b], box[b], m["img_shape"], m["scale_factor"], rescale, K)
        o32, _ = R.get_bboxes_single(cls[b], box[b], m["img_shape"], m["scale_factor"], rescale, K,
                                     dtype=torch.float32)
        assert torch.equal(labels[b].cpu(), rl), case
        assert torch.equal(idx[b].cpu() // C, torch.div(idx[b].cpu(), C, rounding_mode="floor"))
        qi = idx[b].cpu() // C
        bx = box[b][qi].double()
        h, w = m["img_shape"][:2]
        sf = torch.tensor(m["scale_factor"], dtype=torch.float64) if rescale else torch.ones(4, dtype=torch.float64)
        wh = torch.tensor([w, h, w, h], dtype=torch.float64)
        bmag = (bx[:, [0, 1, 0, 1]].abs() + 0.5 * bx[:, [2, 3, 2, 3]].abs()) * wh / sf
        mag = torch.cat([bmag, ref[:, 4:]], -1)
        _note("k_det_results", _bounded("k_det_results", case + " image %d" % b, det[b], ref, mag,
                                        L_RES, o32.to(DEV)), case)
    return det, labels, idx


@pytest.mark.parametrize("rescale", [False, True])
def test_results_config_shape(hip, rescale):
    det, labels, _ = _results_case(hip, 2, 100, 150, 100, rescale, 60)
    d0 = det[0, 0].cpu()
    w = 160.0 / (1.25 if rescale else 1.0)
    assert float(d0[2]) == pytest.approx(w, rel=1e-6) and float(d0[1]) == 0.0    # clamped
    assert int(labels[0, 0]) == 0


@pytest.mark.parametrize("rescale", [False, True])
def test_results_tiny_with_planted_ties(hip, rescale):
    det, labels, idx = _results_case(hip, 2, 2, 3, 4, rescale, 61, ties=True)
    # image 0: 11.0 at flat 0 first, then the three 9.0 in flat-index order
    assert idx[0].tolist() == [0, 1, 4, 5] and labels[0].tolist() == [0, 1, 1, 2]


def test_results_refusals_and_bad_index(hip):
    B, Q, C, K = 1, 2, 3, 4
    cls, box = torch.zeros(B, Q, C, device=DEV), torch.full((B, Q, 4), 0.5, device=DEV)
    meta = torch.tensor([[10.0, 20.0, 1.0, 1.0, 1.0, 1.0]], device=DEV)
    idx = torch.tensor([[0, 6, -1, 5]], dtype=torch.int64, device=DEV)
    det = torch.full((B, K, 5), 3.0, device=DEV)
    labels = torch.full((B, K), 9, dtype=torch.int64, device=DEV)
    hip.det_results(cls, box, idx, meta, det, labels, False)
    torch.cuda.synchronize()
    assert labels[0].tolist() == [0, -1, -1, 2]
    assert bool(torch.isnan(det[0, 1:3]).all()) and bool(torch.isfinite(det[0, [0, 3]]).all())
    lib, P = hip.lib(), hip._ptr
    s = torch.cuda.current_stream().cuda_stream

    def raw(c=cls, b=box, i=idx, m=meta, d=det, l=labels, shape=(B, Q, C, K)):
        pt = lambda t, dt=torch.float32: None if t is None else P(t, dt)
        return lib.pn_det_results_f32(pt(c), pt(b), pt(i, torch.int64), pt(m), pt(d),
                                      pt(l, torch.int64), *shape, 0, s)
    det.fill_(3.0)
    for kw in (dict(c=None), dict(b=None), dict(i=None), dict(m=None), dict(d=None), dict(l=None),
               dict(shape=(0, Q, C, K)), dict(shape=(B, 0, C, K)), dict(shape=(B, Q, 0, K)),
               dict(shape=(B, Q, C, 0)), dict(shape=(B, Q, 257, K)), dict(shape=(B, Q, C, 7)),
               dict(shape=(B, 65537, 1, K))):
        assert raw(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((det == 3.0).all())


# ================================================================== DeformableDETRLoss
@pytest.fixture(scope="module")
def ref_cases():
    """The float64 references of the committed cases, computed once and shared."""
    out = {}
    for name, kw in R.CASES.items():
        case = R.make_case(**kw)
        ok, pairs = R.separated(case)
        assert ok
        vals, _, grads = R.loss(case, grads=True, pairs=pairs)
        v32, _, g32 = R.loss(case, dtype=torch.float32, grads=True, pairs=pairs)   # the fp32 oracle
        out[name] = (case, vals, pairs, grads, v32, g32)
    return out


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_loss_object_against_the_float64_statement(hip, ref_cases, name):
    from pairnet_amd import DeformableDETRLoss, det_train_cfg
    case, vals, pairs, gref, v32, g32 = ref_cases[name]
    L, B, Q, C = case["cls"].shape
    SN = case["enc_cls"].shape[1]
    T = L + 1
    lo = DeformableDETRLoss(C, train_cfg=det_train_cfg())
    dev = {k: case[k].to(DEV) for k in ("cls", "bbox", "enc_cls", "enc_bbox")}
    runs = []
    for _ in range(2):
        grads, trace = {}, []
        got = lo.loss(dev["cls"], dev["bbox"], dev["enc_cls"], dev["enc_bbox"], case["gt_bboxes"],
                      case["gt_labels"], case["img_metas"], grads=grads, trace=trace)
        torch.cuda.synchronize()
        runs.append((got, {k: v.clone() for k, v in grads.items()}, trace))
    got, grads, trace = runs[0]
    for k in grads:
        assert torch.equal(grads[k].view(torch.int32), runs[1][1][k].view(torch.int32)), k
    assert list(got) == R.keys(L) and len(got) == 3 * T
    assert all(v.dim() == 0 and v.is_cuda for v in got.values())
    # ---- the pairs are the reference's ----
    want = [(t, b, pairs[t][b]) for t in range(T) for b in range(B) if pairs[t][b] is not None]
    assert [(e["term"], e["image"]) for e in trace] == [(t, b) for t, b, _ in want]
    for e, (_, _, (r, c)) in zip(trace, want):
        assert np.array_equal(e["rows"], r) and np.array_equal(e["cols"], c)
        assert tuple(e["cost"].shape) == ((Q if e["term"] < L else SN), len(case["gt_labels"][e["image"]]))
    # ---- values and gradients, term by term ----
    Gs = [len(g) for g in case["gt_labels"]]
    rows = L * B * Q + B * SN
    nwg = math.ceil(rows * C / 4096)
    shapes = {"cls": (L, B, Q, C), "bbox": (L, B, Q, 4), "enc_cls": (B, SN, C), "enc_bbox": (B, SN, 4)}
    for k, shp in shapes.items():
        assert tuple(grads[k].shape) == shp and bool(torch.isfinite(grads[k]).all()), k
    f_all = torch.tensor([[m["img_shape"][1], m["img_shape"][0]] * 2 for m in case["img_metas"]],
                         dtype=torch.float64)
    for t in range(T):
        n = Q if t < L else SN
        pre = "" if t == L - 1 else ("enc_" if t == L else "d%d." % t)
        avg = float(max(sum(min(n, g) for g in Gs), 1))
        ref = vals[pre + "loss_cls"]
        _note("loss_cls", _bounded("loss_cls", "%s term %d" % (name, t), got[pre + "loss_cls"].view(1),
                                   ref.view(1), ref.abs().view(1), _focal_sum_L(T, nwg),
                                   v32[pre + "loss_cls"].view(1).to(DEV)), name)
        gk, gb = ("cls", "bbox") if t < L else ("enc_cls", "enc_bbox")
        gc = grads[gk][t] if t < L else grads[gk]
        rc = gref[gk][t] if t < L else gref[gk]
        rc32 = g32[gk][t] if t < L else g32[gk]
        _note("grad cls", _bounded("grad " + gk, "%s term %d" % (name, t), gc, rc, rc.abs(),
                                   L_FOCAL_GRAD, rc32.to(DEV)), name)
        pr, gtb, fa, where = [], [], [], []
        for b in range(B):
            if pairs[t][b] is None:
                continue
            r, c = pairs[t][b]
            src = case["bbox"][t, b] if t < L else case["enc_bbox"][b]
            pr.append(src[torch.from_numpy(r)].double())
            gtb.append(case["gt_bboxes"][b][torch.from_numpy(c)].double())
            fa.append(f_all[b].view(1, 4).expand(len(r), 4))
            where += [(b, int(i)) for i in r]
        gbox = grads[gb][t] if t < L else grads[gb]
        rbox = gref[gb][t] if t < L else gref[gb]
        rbox32 = g32[gb][t] if t < L else g32[gb]
        hit = torch.zeros(B, n, dtype=torch.bool)
        if pr:
            t64 = R.box_pair_terms(torch.cat(pr), torch.cat(gtb), torch.cat(fa))
            m = len(where)
            extra = math.ceil(m / 256) + 11
            for key, kk, w, Lk in (("l1", "loss_bbox", 5.0, L_L1), ("gl", "loss_iou", 2.0, L_GIOU)):
                ref = vals[pre + kk]
                assert abs(float(ref) - w * float(t64[key].val.sum()) / avg) <= 1e-12 * float(ref)
                mag = w * t64[key].mag.sum() / avg
                _note(kk, _bounded(kk, "%s term %d" % (name, t), got[pre + kk].view(1), ref.view(1),
                                   mag.view(1), Lk + extra, v32[pre + kk].view(1).to(DEV)), name)
            bi = torch.tensor([w_[0] for w_ in where])
            ri = torch.tensor([w_[1] for w_ in where])
            hit[bi, ri] = True
            gmag = 5.0 / avg + 2.0 / avg * t64["d_gl"].mag
            _note("grad bbox", _bounded("grad " + gb, "%s term %d" % (name, t),
                                        gbox[bi.to(DEV), ri.to(DEV)], rbox[bi, ri], gmag, L_BOX_GRAD,
                                        rbox32[bi, ri].to(DEV)), name)
        else:
            assert float(got[pre + "loss_bbox"]) == 0.0 and float(got[pre + "loss_iou"]) == 0.0
        assert bool((gbox.cpu()[~hit] == 0).all()) and bool((rbox[~hit] == 0).all())
