"""GPU: `pn_box_match_cost_f32` (csrc/box_loss.hip) against the float64 statement
`bbox_loss_ref.cost_terms`, and `CrossHeadBBox`'s loss (pair-net_amd/bbox_losses.py) against the
fixture tests/golden/bbox_loss.npz (the reference's own `CrossHeadBBox.loss`, recorded by
tools/make_bbox_loss_golden.py).

Bounds: the rule of tests/test_loss_optim_kernels_gpu.py -- |got - ref| <= c 2^-24 mag + FLT_MIN,
c = L + max(4, 2 x the ratio the same statement reaches when torch evaluates it in fp32 on the same
inputs against its own float64 run); nothing of c comes from the kernel under test.

k_box_match_cost, L = 14, the longest chain of fp32 roundings of a cell, counted from the source:
  cls   expf 1, 1 + e 1, 1 / . 1 (p), 1 - p 1, + eps 1, logf 1, 1 - alpha 1, * 1, p p 1, * 1
        (neg: 10; pos is shorter), pos - neg 1, * w 1                                     = 12
  reg   gt / f 1, x1 + x2 1 (/ 2 exact), box - . 1, three adds 3, * w 1                   =  7
  iou   0.5 w exact, cx -+ . 1, * f 1, x2 - x1 1, area 1, area1 + area2 1, - overlap 1,
        overlap / union 1, enclose - union 1, / 1, iou - . 1, * w 1                       = 11
  cost  the longest term + the two final adds                                             = 14
The magnitude (bbox_loss_ref.cost_terms): the focal terms' absolute values with their conditioning
(p = sigmoid(x) is rounded to 2^-24 p, and `1 - p` hands that absolute error to log(1 - p + eps)
and (1 - p)^gamma: p / (1 - p + eps) beside |log|), the reg terms' absolute values (with the
operands of the reg differences) plus, for the GIoU, both areas, the overlap, the union, the
enclosing area and the products of the corner coordinates they are differences of, each divided by
the area it is divided by -- so that the cancellations in `area1 + area2 - overlap` and
`enclose - union` are covered, and a cell whose union is clamped to eps is bounded relative to eps.

The loss values use the L of the reductions they run (tests/test_loss_optim_kernels_gpu.py:
ce_mean ceil(C / 64) + rows + 12 + ceil(ln C + 1); seesaw_mean rows + 32; bce_posw_mean
ceil(n / 1024) + 33) with the fixture's float64 magnitudes; the logit gradients take their tensor's
largest float64 entry as magnitude and L = 40 (the seesaw gradient's chain: the value's 32 + the
softmax of the shifted logits, / n, * lw; the other two are shorter).
"""
import math

import numpy as np
import pytest
import torch

import bbox_loss_ref as R
from test_loss_optim_kernels_gpu import _bounded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
L_COST = 14
FENCE = 8
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


# ================================================================== the cost kernel
def _cost_inputs(Q, Gs, nc, seed):
    """Random boxes and logits with the edge cases planted: logits at +-80; query 0 EQUAL to
    ground truth 0 (exactly representable corners), query 1 of zero area; ground truth 1 of zero
    area, ground truth 2 enclosing query 0; the rest random, most pairs disjoint."""
    g = torch.Generator().manual_seed(seed)
    B = len(Gs)
    cls = torch.randn(B, Q, nc, generator=g) * 3.0
    cls[:, ::3, ::2] = 80.0
    cls[:, 1::3, ::2] = -80.0
    box = torch.cat([torch.rand(B, Q, 2, generator=g) * 0.8 + 0.1,
                     torch.rand(B, Q, 2, generator=g) * 0.2 + 0.01], -1)
    shapes = [(48 + 16 * b, 64 + 32 * ((b + 1) % 2)) for b in range(B)]       # (h, w), non-square
    labels, boxes = [], []
    for b, G in enumerate(Gs):
        h, w = shapes[b]
        f = torch.tensor([w, h, w, h], dtype=torch.float32)
        c, s = torch.rand(G, 2, generator=g) * 0.6 + 0.2, torch.rand(G, 2, generator=g) * 0.3 + 0.05
        gb = torch.cat([c - s / 2, c + s / 2], -1) * f
        box[b, 0] = torch.tensor([0.5, 0.25, 0.25, 0.125])
        gb[0] = torch.tensor([0.375, 0.1875, 0.625, 0.3125]) * f               # == xyxy(box 0) * f
        box[b, 1, 2:] = 0.0
        if G > 1:
            gb[1, 2:] = gb[1, :2]
        if G > 2:
            gb[2] = torch.tensor([0.25, 0.125, 0.75, 0.5]) * f
        labels.append(torch.randint(0, nc, (G,), generator=g))
        boxes.append(gb)
    return cls, box, labels, boxes, shapes


def _launch(hip, cls, box, labels, boxes, shapes, fill=NAN):
    """One launch into a NaN-fenced buffer: FENCE floats in front of, between and behind the
    blocks -> (buffer, [(offset, G)])."""
    B, Q, nc = cls.shape
    tab, where, off, l_off = [], [], FENCE, 0
    for b in range(B):
        G = labels[b].numel()
        tab += [off, G, l_off, l_off]
        where.append((off, G))
        off += Q * G + FENCE
        l_off += G
    cost = torch.full((off,), fill, device=DEV)
    factor = torch.tensor([[w, h, w, h] for h, w in shapes], dtype=torch.float32, device=DEV)
    hip.box_match_cost(cls.to(DEV), box.to(DEV), torch.cat(labels).to(DEV),
                       torch.cat(boxes).to(DEV), factor,
                       torch.tensor(tab, dtype=torch.int64, device=DEV).view(B, 4), cost,
                       max(Q * g for _, g in where), **{k: v for k, v in R.CFG.items()})
    return cost, where


COST_CASES = [(100, (1,), 150, 1), (2, (3, 1), 1, 2), (100, (65, 3, 17), 256, 3),
              (100, (7, 3), 150, 4), (1024, (1024,), 150, 5)]


@pytest.mark.parametrize("Q,Gs,nc,seed", COST_CASES)
def test_box_match_cost(hip, Q, Gs, nc, seed):
    cls, box, labels, boxes, shapes = _cost_inputs(Q, Gs, nc, seed)
    cost, where = _launch(hip, cls, box, labels, boxes, shapes)
    cost2, _ = _launch(hip, cls, box, labels, boxes, shapes)
    torch.cuda.synchronize()
    assert torch.equal(cost.view(torch.int32), cost2.view(torch.int32)), "not bitwise reproducible"
    written = torch.zeros(cost.numel(), dtype=torch.bool)
    for b, (off, G) in enumerate(where):
        h, w = shapes[b]
        f = torch.tensor([w, h, w, h], dtype=torch.float32)
        got = cost[off:off + Q * G].view(Q, G)
        assert bool(torch.isfinite(got).all()), "image %d: non-finite cells" % b
        ref, mag = R.cost_terms(cls[b], box[b], labels[b], boxes[b], f)
        o32, _ = R.cost_terms(cls[b], box[b], labels[b], boxes[b], f, dtype=torch.float32)
        case = "Q %d G %d nc %d image %d" % (Q, G, nc, b)
        _note("k_box_match_cost", _bounded("k_box_match_cost", case, got, ref, mag, L_COST,
                                           o32.to(DEV)), case)
        # the planted cells: equal boxes have GIoU 1 to rounding; the clamps give finite values
        giou = R.giou_parts(R.bbox_cxcywh_to_xyxy(box[b].double()) * f.double(), boxes[b].double())[0]
        assert float(giou[0, 0]) == 1.0
        written[off:off + Q * G] = True
    assert bool(torch.isnan(cost.cpu()[~written]).all()), "wrote outside its blocks"


def test_box_match_cost_refusals_leave_the_fences(hip):
    cls, box, labels, boxes, shapes = _cost_inputs(100, (3, 2), 7, 11)
    B, Q, nc = cls.shape
    fence = torch.full((100 * 5 + 64,), NAN, device=DEV)
    args = dict(cls=cls.to(DEV), box=box.to(DEV), gt_labels=torch.cat(labels).to(DEV),
                gt_bboxes=torch.cat(boxes).to(DEV),
                factor=torch.tensor([[w, h, w, h] for h, w in shapes], dtype=torch.float32, device=DEV),
                tab=torch.tensor([[0, 3, 0, 0], [300, 2, 3, 3]], dtype=torch.int64, device=DEV),
                cost=fence, max_cells=300)
    lib = hip.lib()
    P = lambda t, d=torch.float32: hip._ptr(t, d)

    def raw(**over):
        a = dict(args, **over)
        Bq, Qq, ncq = a.get("shape", (B, Q, nc))
        return lib.pn_box_match_cost_f32(
            P(a["cls"]), P(a["box"]), P(a["gt_labels"], torch.int64), a["gt_labels"].numel(),
            P(a["gt_bboxes"]), a["gt_bboxes"].shape[0], P(a["factor"]), P(a["tab"], torch.int64),
            P(a["cost"]), fence.numel(), a["max_cells"], Bq, Qq, ncq, 2.0, 5.0, 2.0, 0.25, 2.0,
            1e-12, 1e-6, torch.cuda.current_stream().cuda_stream)
    # (the null pointers stand for all seven; G = 0 everywhere is max_cells = 0 on the host side)
    for over in (dict(cls=None), dict(tab=None), dict(cost=None), dict(max_cells=0),
                 dict(shape=(B, 1, nc)), dict(shape=(B, Q, 257)), dict(shape=(0, Q, nc))):
        assert raw(**over) == -1, over
    # G = 0 / a block past the buffer / labels past theirs, in the DEVICE table: that image's block
    # is left alone, the other image's is written
    for row in ([0, 0, 0, 0], [400, 2, 3, 3], [0, 3, 3, 0], [0, 3, 0, 3], [-1, 3, 0, 0], [0, 1025, 0, 0]):
        tab = torch.tensor([row, [300, 2, 3, 3]], dtype=torch.int64, device=DEV)
        assert raw(tab=tab) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(fence[:300]).all()) and bool(torch.isnan(fence[500:]).all()), row
        assert bool(torch.isfinite(fence[300:500]).all()), row
        fence.fill_(NAN)
    torch.cuda.synchronize()
    assert bool(torch.isnan(fence).all())
    # a label outside [0, nc): NaN cells (pn_lsa_f32 status 1), nothing else disturbed
    bad = torch.cat(labels).to(DEV)
    bad[1] = nc
    assert raw(gt_labels=bad) == 0
    torch.cuda.synchronize()
    blk = fence[:300].view(100, 3)
    assert bool(torch.isnan(blk[:, 1]).all()) and bool(torch.isfinite(blk[:, [0, 2]]).all())


# ================================================================== the loss
HEAD = {}


def _loss_obj(case):
    from pairnet_amd.bbox_losses import CrossHeadBBoxLoss
    return CrossHeadBBoxLoss(case["num_classes"], case["num_relations"], case["rel"].shape[1],
                             subobj_cls_loss=dict(type="CrossEntropyLoss", use_sigmoid=False,
                                                  loss_weight=4.0, reduction="mean",
                                                  class_weight=[1.0] * case["num_classes"]))


def _run(case, device_targets, mutate=None):
    loss = _loss_obj(case)
    d = lambda k: case[k].to(DEV)
    cls = dict(cls=d("cls"), sub=d("sub"), obj=d("obj"), rel=d("rel"), importance=d("importance"))
    box = dict(bbox=d("bbox"))
    if mutate is not None:
        mutate(cls, box)
    grads, trace = {}, []
    out = loss.loss(cls, box, case["gt_rels"], case["gt_bboxes"], case["gt_labels"],
                    case["img_metas"], grads=grads, trace=trace, device_targets=device_targets)
    torch.cuda.synchronize()
    return out, grads, trace, loss


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_loss_against_the_fixture(hip, name):
    case, ref = R.golden_case(name)
    host = _run(case, False)
    dev = _run(case, True)
    B, Rq = case["rel"].shape[:2]
    nc, C = case["num_classes"], case["num_relations"]
    for mode, (out, grads, trace, loss) in (("host", host), ("device", dev)):
        for b in range(B):
            for k in ("box_rows", "box_cols", "triplet_rows", "triplet_cols"):
                assert np.array_equal(np.asarray(trace[b][k]), ref["%s.%d" % (k, b)]), (mode, k, b)
        if mode == "device":
            assert int(loss.assign_status.cpu()) == 0
        rows = B * Rq
        Ls = dict(loss_sub_cls=math.ceil(nc / 64) + rows + 12 + math.ceil(math.log(nc) + 1.0),
                  loss_r_cls=rows + 32, loss_match=math.ceil(B * 100 * 100 / 1024) + 33)
        Ls["loss_obj_cls"] = Ls["loss_sub_cls"]
        assert set(out) == set(Ls)
        for k, L in Ls.items():
            f64 = torch.tensor(float(ref[k + ".f64"]), dtype=torch.float64, device=DEV)
            o32 = torch.tensor(float(ref[k + ".f32"]), device=DEV)
            mag = torch.tensor(float(ref[k + ".mag"]), dtype=torch.float64)
            case_s = "%s %s %s" % (name, mode, k)
            _note(k, _bounded(k, case_s, out[k].reshape(()), f64, mag, L, o32), case_s)
        for k in ("rel", "importance", "sub", "obj"):
            f64 = torch.from_numpy(ref["grad.%s.f64" % k])
            o32 = torch.from_numpy(ref["grad.%s.f32" % k]).to(DEV)
            mag = torch.full(f64.shape, float(ref["grad.%s.mag" % k]), dtype=torch.float64)
            case_s = "%s %s d %s" % (name, mode, k)
            _note("d " + k, _bounded("d " + k, case_s, grads[k], f64, mag, 40, o32), case_s)
    # the device mode gives bitwise the host mode's losses and gradients
    for k in host[0]:
        assert torch.equal(host[0][k], dev[0][k]), k
    for k in host[1]:
        assert torch.equal(host[1][k], dev[1][k]), k
    assert np.array_equal(host[3].cum_samples, dev[3].cum_samples)


def test_planted_nan_sets_the_status_without_an_exception(hip):
    case, _ = R.golden_case("a")

    def plant(cls, box):
        box["bbox"][1, 17, 2] = NAN
    out, grads, trace, loss = _run(case, True, plant)
    assert int(loss.assign_status.cpu()) != 0
    assert float(loss.cum_samples.sum()) == 0.0          # counts untouched
    with pytest.raises(ValueError):                       # the host path raises, as scipy does
        _run(case, False, plant)


def test_quirks(hip):
    case, _ = R.golden_case("b")
    G = case["gt_labels"][0].numel()
    # (1) the importance target sits at (query of the subject box, query of the object box):
    # d loss_match / d importance is negative exactly where the target is 1
    for mode in (False, True):
        out, grads, trace, loss = _run(case, mode)
        q_of = np.ones(G, dtype=np.int64)
        q_of[trace[0]["box_cols"]] = trace[0]["box_rows"]
        rels = case["gt_rels"][0].numpy()
        tgt = np.zeros((100, 100), np.float32)
        tgt[q_of[rels[:, 0]], q_of[rels[:, 1]]] = 1.0
        neg = (grads["importance"][0] < 0).cpu().numpy()
        assert np.array_equal(neg, tgt > 0), mode
    # (2) a duplicate (subject, object) pair gives importance 1, not 2: the loss of the batch with
    # the pair doubled equals, bit for bit in loss_match, the batch without the copy
    dup = dict(case, gt_rels=[torch.cat([case["gt_rels"][0], case["gt_rels"][0][:1]], 0)])
    for mode in (False, True):
        a, b = _run(case, mode), _run(dup, mode)
        assert torch.equal(a[0]["loss_match"], b[0]["loss_match"]), mode
        assert torch.equal(a[1]["importance"], b[1]["importance"]), mode
    # (3) an unmatched object points at query 1.  Unmatched needs G > Q: 101 boxes, and the
    # relation's subject is whichever box stays unmatched
    many = R.make_case(seed=4, G=(101,), T=(1,), planted=False)
    for mode in (False, True):
        out, grads, trace, loss = _run(many, mode)
        un = sorted(set(range(101)) - set(int(c) for c in trace[0]["box_cols"]))
        assert len(un) == 1
        q_of = np.ones(101, dtype=np.int64)
        q_of[trace[0]["box_cols"]] = trace[0]["box_rows"]
        case2 = dict(many, gt_rels=[torch.tensor([[un[0], (un[0] + 1) % 101, 1]])])
        out2, grads2, trace2, _ = _run(case2, mode)
        neg = torch.nonzero(grads2["importance"][0] < 0).cpu().numpy()
        assert neg.shape == (1, 2) and int(neg[0, 0]) == 1, (mode, neg)     # subject -> query 1
        assert int(neg[0, 1]) == int(q_of[(un[0] + 1) % 101])
    # (4) an image without relations
    empty = dict(case, gt_rels=[case["gt_rels"][0][:0]])
    for mode in (False, True):
        with pytest.raises(ValueError):
            _run(empty, mode)
