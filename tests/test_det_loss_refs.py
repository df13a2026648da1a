"""CPU: the float64 statements of tests/det_loss_ref.py pinned without a GPU, the committed cases'
assignments separated, and the plain detector's declarations, refusals and construction.

Pins: the focal element and the L1 / GIoU sums against `transformers.loss.loss_for_object_detection`
(an independent DETR loss; non-degenerate boxes, where mmdet's 1e-6 clamps do not act; `num_boxes`
set to the same factor), the match cost against tests/bbox_loss_ref.py's statement, the closed-form
gradients against autograd through the float64 statements."""
import os
import re

import numpy as np
import pytest
import torch

import bbox_loss_ref as BR
import det_loss_ref as R

ENTRIES = ("pn_det_match_cost_f32", "pn_det_focal_f32", "pn_det_box_loss_f32", "pn_det_results_f32")


# ------------------------------------------------------------------------ pins of the statements
def test_focal_element_against_transformers_and_mmdets_literal_form():
    from transformers.loss.loss_for_object_detection import sigmoid_focal_loss
    g = torch.Generator().manual_seed(0)
    rows, C = 37, 11
    x = torch.randn(rows, C, generator=g, dtype=torch.float64) * 3.0
    labels = torch.randint(0, C + 1, (rows,), generator=g)         # C = background
    onehot = (labels.view(-1, 1) == torch.arange(C).view(1, -1)).double()
    el = R.focal_elements(x, labels, 0.25, 2.0)
    # (the literal form's `1 - p` carries float64's rounding of p relative to pt = 1 - p: the
    # tolerance is that conditioning, gamma + 1 times, beside a plain 1e-14)
    pt = torch.sigmoid(torch.where(onehot.bool(), -x, x))
    tol = lambda gamma: el.abs() * (1e-14 + (gamma + 1) * 2.0 ** -52 / pt)
    assert bool(((el - R.py_sigmoid_focal_loss(x, onehot, 0.25, 2.0)).abs() <= tol(2.0)).all())
    for num_boxes in (1.0, 7.0):
        hf = sigmoid_focal_loss(x.view(rows, 1, C), onehot.view(rows, 1, C), num_boxes, 0.25, 2.0)
        assert abs(float(hf) - float(el.sum() / num_boxes)) <= float(tol(2.0).sum()) / num_boxes
    # element by element: one element per call
    for r, c in ((0, 0), (5, 3), (36, 10)):
        hf = sigmoid_focal_loss(x[r:r + 1, c:c + 1].view(1, 1, 1), onehot[r:r + 1, c:c + 1].view(1, 1, 1),
                                1.0, 0.25, 2.0)
        assert abs(float(hf) - float(el[r, c])) <= float(tol(2.0)[r, c])
    # other alpha / gamma
    el2 = R.focal_elements(x, labels, 0.4, 1.5)
    tol2 = el2.abs() * (1e-14 + 2.5 * 2.0 ** -52 / pt)
    assert bool(((el2 - R.py_sigmoid_focal_loss(x, onehot, 0.4, 1.5)).abs() <= tol2).all())


def test_l1_and_giou_sums_against_transformers():
    from transformers.loss.loss_for_object_detection import generalized_box_iou
    g = torch.Generator().manual_seed(1)
    n = 23
    pred = torch.cat([torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.6 + 0.2,
                      torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.3 + 0.05], -1)
    f = torch.tensor([[160.0, 112.0, 160.0, 112.0]], dtype=torch.float64).expand(n, 4)
    c = torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.6 + 0.2
    s = torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.3 + 0.05
    gt = torch.cat([c - s / 2, c + s / 2], -1) * f
    l1, gi = R.box_terms(pred, gt, f)
    target = R.xyxy_to_cxcywh(gt / f)
    assert abs(float(l1) - float(torch.nn.functional.l1_loss(pred, target, reduction="sum"))) < 1e-12
    hf = 1 - torch.diag(generalized_box_iou(R.cxcywh_to_xyxy(pred) * f, gt))
    assert abs(float(gi) - float(hf.sum())) <= 1e-11 * float(hf.sum())


def test_cost_against_bbox_loss_refs_statement():
    for Q, G, nc, seed in ((100, 7, 150, 0), (1024, 3, 11, 1), (2, 1, 1, 2)):
        g = torch.Generator().manual_seed(seed)
        cls = torch.randn(Q, nc, generator=g) * 3.0
        box = torch.cat([torch.rand(Q, 2, generator=g) * 0.8 + 0.1,
                         torch.rand(Q, 2, generator=g) * 0.2 + 0.01], -1)
        f = torch.tensor([96.0, 64.0, 96.0, 64.0])
        c, s = torch.rand(G, 2, generator=g) * 0.6 + 0.2, torch.rand(G, 2, generator=g) * 0.3 + 0.05
        gt = torch.cat([c - s / 2, c + s / 2], -1) * f
        gl = torch.randint(0, nc, (G,), generator=g)
        want, mag = BR.cost_terms(cls, box, gl, gt, f)
        got = R.match_cost(cls, box, gl, gt, f)
        assert bool(((got - want).abs() <= 1e-13 * mag).all())


def test_gradients_against_autograd():
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(9, 5, generator=g, dtype=torch.float64) * 4.0).requires_grad_(True)
    labels = torch.tensor([0, 5, 4, 5, 2, 5, 5, 1, 3])
    R.focal_elements(x, labels, 0.25, 2.0).sum().backward()
    assert torch.allclose(x.grad, R.focal_grad(x.detach(), labels, 0.25, 2.0), rtol=1e-12, atol=1e-300)
    case = R.make_case(7, L=2, B=2, Q=6, C=5, SN=20, Gs=(3, 0))
    vals, pairs, gr = R.loss(case, grads=True)
    assert sorted(vals) == sorted(R.keys(2)) and len(vals) == 9
    assert all(bool(torch.isfinite(v)) for v in vals.values())
    # every unmatched box row has a zero gradient; matched rows do not
    for i in range(3):
        gb = gr["bbox"][i] if i < 2 else gr["enc_bbox"]
        r, _ = pairs[i][0]
        hit = torch.zeros(gb.shape[1], dtype=torch.bool)
        hit[torch.from_numpy(r)] = True
        assert bool((gb[0][~hit] == 0).all()) and bool((gb[0][hit].abs().sum(-1) > 0).all())
        assert bool((gb[1] == 0).all())                    # the image without ground truth
    # the class gradient is the closed form scaled by w_cls / avg_factor
    (_, _, _), _, _, labels0 = R.loss_single(case["cls"][0], case["bbox"][0], case["gt_bboxes"],
                                              case["gt_labels"], case["img_metas"])
    want = R.focal_grad(case["cls"][0].double().reshape(-1, 5), labels0.view(-1)) * (2.0 / 3.0)
    assert torch.allclose(gr["cls"][0].reshape(-1, 5), want, rtol=1e-12, atol=1e-300)


def test_box_pair_terms_against_the_statements_and_autograd():
    g = torch.Generator().manual_seed(4)
    n = 40
    pred = torch.cat([torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.6 + 0.2,
                      torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.3 + 0.05], -1)
    f = torch.tensor([[160.0, 112.0, 160.0, 112.0]], dtype=torch.float64).expand(n, 4).contiguous()
    c = torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.6 + 0.2
    s = torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.3 + 0.05
    gt = torch.cat([c - s / 2, c + s / 2], -1) * f
    pred[0] = torch.tensor([0.5, 0.5, 0.2, 0.2])                         # nested in gt 0
    gt[0] = torch.tensor([0.3, 0.3, 0.8, 0.8]) * f[0]
    pred[1] = torch.tensor([0.2, 0.2, 0.1, 0.1])                         # disjoint from gt 1
    gt[1] = torch.tensor([0.6, 0.6, 0.9, 0.9]) * f[1]
    pred.requires_grad_(True)
    l1, gi = R.box_terms(pred, gt, f)
    t = R.box_pair_terms(pred.detach(), gt, f)
    assert abs(float(l1.detach()) - float(t["l1"].val.sum())) < 1e-12
    assert abs(float(gi.detach()) - float(t["gl"].val.sum())) < 1e-12
    assert bool((t["gl"].mag >= t["gl"].val.abs()).all())
    (d1,) = torch.autograd.grad(l1, pred, retain_graph=True)
    (d2,) = torch.autograd.grad(gi, pred)
    assert torch.equal(d1, t["d_l1"])
    assert bool(((d2 - t["d_gl"].val).abs() <= 1e-13 * t["d_gl"].mag).all())
    assert bool((t["d_gl"].mag >= t["d_gl"].val.abs() * (1 - 1e-12)).all())


def test_zero_ground_truth_everywhere_and_more_boxes_than_rows():
    case = R.make_case(11, L=1, B=2, Q=4, C=3, SN=9, Gs=(0, 0))
    vals, pairs, _ = R.loss(case)
    assert float(vals["loss_bbox"]) == 0.0 and float(vals["enc_loss_iou"]) == 0.0
    assert float(vals["loss_cls"]) > 0.0                   # all background, factor clamped to 1
    case = R.make_case(12, L=1, B=1, Q=4, C=3, SN=9, Gs=(6,))
    vals, pairs, _ = R.loss(case)
    assert len(pairs[0][0][0]) == 4 and len(pairs[1][0][0]) == 6


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_committed_cases_have_separated_assignments(name):
    case = R.make_case(**R.CASES[name])
    ok, pairs = R.separated(case)
    assert ok, "case %s: the fp32 cost gives other pairs than the float64 cost" % name
    L = case["cls"].shape[0]
    assert len(pairs) == L + 1


def test_get_bboxes_single_statement():
    cls = torch.tensor([[0.5, -1.0, 2.0], [2.0, 0.25, -3.0]])          # a tie at 2.0
    box = torch.tensor([[0.5, 0.5, 0.5, 0.5], [0.9, 0.9, 0.4, 0.4]])
    det, labels = R.get_bboxes_single(cls, box, (100, 200, 3), [2.0, 2.0, 2.0, 2.0], True, 4)
    assert labels.tolist() == [2, 0, 0, 1]                             # tie: flat 2 before flat 3
    assert torch.allclose(det[0, :4], torch.tensor([25.0, 12.5, 75.0, 37.5], dtype=torch.float64))
    assert torch.allclose(det[1, :4], torch.tensor([70.0, 35.0, 100.0, 50.0], dtype=torch.float64))
    res = R.bbox2result(det.numpy(), labels.numpy(), 3)
    assert [len(r) for r in res] == [2, 1, 1]


# ------------------------------------------------------------------------ declarations
def test_entries_are_declared_bound_exported_and_listed():
    from pairnet_amd import build as B
    from pairnet_amd import hip
    header = open(os.path.join(B.ROOT, "include", "pairnet_hip.h")).read()
    assert re.search(r"#define PN_ABI_VERSION 34\b", header) and hip.ABI_VERSION == 34
    for name in ENTRIES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int64_t pn_det_focal_partials[^;]*;\s*)?int %s\("
                      % name, header, re.S)
        assert m, "%s is not declared behind a comment" % name
        assert "od_r101_vg.py:" in m.group(1) and "pairnet_bbox_head.py:596-642" in m.group(1), name
        assert name in hip._SIGS and name in hip.EXPORTS, name
    assert "det_loss" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "det_loss.hip"))
    for fn in ("det_match_cost", "det_focal", "det_box_loss", "det_results"):
        assert callable(getattr(hip, fn))


# ------------------------------------------------------------------------ construction / refusals
def test_loss_construction_refusals():
    from pairnet_amd import DeformableDETRLoss, det_train_cfg
    ok = DeformableDETRLoss(150, train_cfg=det_train_cfg())
    assert (ok.w_cls, ok.w_bbox, ok.w_iou) == (2.0, 5.0, 2.0) and ok.cost_w == (2.0, 5.0, 2.0)
    assert (ok.alpha, ok.gamma) == (0.25, 2.0)
    custom = DeformableDETRLoss(
        7, loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=1.5, alpha=0.4, loss_weight=1.0),
        loss_bbox=dict(type="L1Loss", loss_weight=3.0), loss_iou=dict(type="GIoULoss", loss_weight=4.0),
        train_cfg=dict(assigner=dict(type="HungarianAssigner",
                                     cls_cost=dict(type="FocalLossCost", weight=1.0),
                                     reg_cost=dict(type="BBoxL1Cost", weight=2.0, box_format="xywh"),
                                     iou_cost=dict(type="IoUCost", iou_mode="giou", weight=3.0))))
    assert (custom.alpha, custom.gamma, custom.w_cls, custom.w_bbox, custom.w_iou) == \
        (0.4, 1.5, 1.0, 3.0, 4.0) and custom.cost_w == (1.0, 2.0, 3.0)
    a = det_train_cfg()["assigner"]
    bad = [dict(loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True)),
           dict(loss_cls=dict(type="FocalLoss", use_sigmoid=False)),
           dict(loss_bbox=dict(type="SmoothL1Loss")), dict(loss_iou=dict(type="IoULoss")),
           dict(train_cfg=dict(assigner=dict(a, type="MaxIoUAssigner"))),
           dict(train_cfg=dict(assigner=dict(a, cls_cost=dict(type="ClassificationCost")))),
           dict(train_cfg=dict(assigner=dict(a, reg_cost=dict(type="BBoxL1Cost", box_format="xyxy")))),
           dict(train_cfg=dict(assigner=dict(a, iou_cost=dict(type="IoUCost", iou_mode="iou")))),
           dict(device_targets=True), dict(group=object())]
    for kw in bad:
        with pytest.raises(NotImplementedError):
            DeformableDETRLoss(150, **kw)
    x = torch.zeros(1, 1, 2, 150)
    for kw in (dict(device_targets=True), dict(group=object())):
        with pytest.raises(NotImplementedError):
            ok.loss(x, torch.zeros(1, 1, 2, 4), torch.zeros(1, 3, 150), torch.zeros(1, 3, 4),
                    [torch.zeros(0, 4)], [torch.zeros(0)], [dict(img_shape=(8, 8, 3))], **kw)


def test_head_refuses_the_forms_that_are_not_built():
    from pairnet_amd import DeformableDETRHead, det_head_cfg
    cfg = dict(det_head_cfg())
    cfg.pop("type")
    for over in (dict(as_two_stage=False), dict(with_box_refine=False),
                 dict(as_two_stage=False, with_box_refine=False)):
        with pytest.raises(NotImplementedError):
            DeformableDETRHead(**dict(cfg, **over))
    head = DeformableDETRHead(**cfg)
    with pytest.raises(NotImplementedError, match="INTEGRATION.md"):
        head.forward_train()


@pytest.mark.parametrize("which,queries,backbone", [("od_r101_vg", 100, "ResNet50Hip"),
                                                    ("od_rnext101_vg", 300, "ResNeXtHip")])
def test_build_detector_returns_the_plain_detector(which, queries, backbone):
    import pairnet_amd as P
    cfg = getattr(P, which)()
    assert cfg.model["type"] == "DeformableDETR"
    det = P.build_detector(cfg.model)
    assert type(det) is P.DeformableDETR and type(det.bbox_head) is P.DeformableDETRHead
    assert type(det.backbone).__name__ == backbone
    head = det.bbox_head
    assert head.num_proposals == head.num_query == queries and head.num_classes == 150
    assert head.test_cfg["max_per_img"] == 100
    keys = list(det.state_dict())
    hk = [k[len("bbox_head."):] for k in keys if k.startswith("bbox_head.")]
    assert any(k.startswith("backbone.") for k in keys) and any(k.startswith("neck.") for k in keys)
    assert all(k.startswith(("transformer.", "cls_branches.", "reg_branches.")) for k in hk)
    assert not any("query_embedding" in k for k in hk)
    for i in range(7):
        assert tuple(head._params["cls_branches.%d.weight" % i].shape) == (150, 256)
        for j, n in ((0, 256), (2, 256), (4, 4)):
            assert tuple(head._params["reg_branches.%d.%d.weight" % (i, j)].shape) == (n, 256)
    assert "cls_branches.7.weight" not in head._params
    for k in ("transformer.level_embeds", "transformer.enc_output.weight",
              "transformer.pos_trans_norm.bias", "transformer.encoder.layers.5.ffns.0.layers.1.bias",
              "transformer.decoder.layers.5.attentions.1.output_proj.weight"):
        assert k in head._params, k
    # the trunk's names are CrossHeadBBox's, one for one
    box = P.build_detector(P.cross_r101_vg().model).bbox_head
    trunk = [k for k in box._params if k.startswith(("transformer.", "cls_branches.", "reg_branches."))]
    assert trunk == list(head._params)
    # the loss is built from the config's own numbers
    lo = head.loss_object()
    assert (lo.w_cls, lo.w_bbox, lo.w_iou, lo.alpha, lo.gamma) == (2.0, 5.0, 2.0, 0.25, 2.0)
    assert lo.cost_w == (2.0, 5.0, 2.0)
    # detect() uses the od configs' own test pipeline (vg_detection.py: Pad to a multiple of 32)
    pad = [t for t in P.det_test_pipeline_cfg()[1]["transforms"] if t["type"] == "Pad"][0]
    assert pad["size_divisor"] == 32 and P.det_test_pipeline_cfg()[1]["img_scale"] == (1333, 800)
    from pairnet_amd import hip
    assert (hip.DET_MAX_G, hip.DET_MAX_ROWS, hip.DET_MAX_TERMS) == (1024, 65536, 16)
    # PSGTr keeps refusing this head type
    with pytest.raises(NotImplementedError):
        P.build_detector(dict(cfg.model, type="PSGTr"))
