"""No GPU: what the box head's loss tests stand on (tests/bbox_loss_ref.py).

  (1) the float64 restatement of `_get_target_single` + `loss_single` equals the reference's own
      `CrossHeadBBox.loss`, run in place through oracle/ref_shim with the restated [3P] assigner /
      sampler patched onto the loaded module: values and autograd gradients to 1e-12 (skipped
      where the reference tree is absent);
  (2) the fixture tests/golden/bbox_loss.npz: its float64 values are what the restatement gives
      today, its assignments have a margin above 1e-3 (as tests/test_loss_optim_refs.py requires
      of the mask cost), its fp32 and float64 runs assign alike;
  (3) the cost statement `cost_terms` is `HungarianAssigner.cost`, and its magnitude dominates
      every term;
  (4) the new entry is declared, bound, built and refuses bad arguments without launching; the
      head accepts `train_cfg` and refuses what the loss does not cover.
"""
import os
import re

import numpy as np
import pytest
import torch

import bbox_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref_available():
    from oracle import ref_shim
    return ref_shim.available()


needs_reference = pytest.mark.skipif(not _ref_available(), reason="reference tree absent")
CASES = dict(R.GOLDEN_CASES, random=dict(seed=5, G=(4, 2), T=(3, 5), planted=False))


# ------------------------------------------------------------------- (1) pinned to the reference
@needs_reference
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference_in_float64(name):
    case = R.make_case(**CASES[name])
    ref, g_ref, assigned = R.run_reference(case, torch.float64)
    got, traces, g = R.loss(case, torch.float64, grads=True)
    assert set(ref) == {"loss_r_cls", "loss_sub_cls", "loss_obj_cls", "loss_match"}
    for k in ref:
        assert abs(float(ref[k]) - float(got[k])) <= 1e-12 * max(1.0, abs(float(ref[k]))), k
    for k in g_ref:
        scale = max(1.0, float(g_ref[k].abs().max()))
        assert float((g_ref[k] - g[k]).abs().max()) <= 1e-12 * scale, k
    # the reference's AssignResults (box matcher, id matcher per image) are the restated pairs
    for b, tr in enumerate(traces):
        box, tri = assigned[2 * b], assigned[2 * b + 1]
        rows = torch.nonzero(box > 0).squeeze(-1)
        assert np.array_equal(rows.numpy(), tr["box_rows"])
        assert np.array_equal((box[rows] - 1).numpy(), tr["box_cols"])
        rows = torch.nonzero(tri > 0).squeeze(-1)
        assert np.array_equal(rows.numpy(), tr["triplet_rows"])
        assert np.array_equal((tri[rows] - 1).numpy(), tr["triplet_cols"])


@needs_reference
def test_reference_rejects_an_image_without_relations():
    case = R.make_case(**R.GOLDEN_CASES["b"])
    case["gt_rels"][0] = case["gt_rels"][0][:0]
    with pytest.raises(Exception):
        R.run_reference(case, torch.float64)
    with pytest.raises(ValueError):
        R.loss(case, torch.float64)


# ------------------------------------------------------------------------------ (2) the fixture
@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_fixture_is_current_and_its_assignments_have_a_margin(name):
    from pairnet_amd import hip
    assert callable(getattr(hip, "box_match_cost", None)), "the fixture is for hip.box_match_cost"
    case, ref = R.golden_case(name)
    spec = R.GOLDEN_CASES[name]
    B = len(spec["G"])
    assert case["cls"].shape[0] == B
    assert [int(g.shape[0]) for g in case["gt_bboxes"]] == list(spec["G"])
    assert [int(r.shape[0]) for r in case["gt_rels"]] == list(spec["T"])
    if name == "b":     # img_shape inside the batch shape
        h, w = case["img_metas"][0]["img_shape"][:2]
        bh, bw = case["img_metas"][0]["batch_input_shape"]
        assert h < bh and w < bw
    fresh = R.make_case(**spec)
    for k in ("cls", "bbox", "sub", "obj", "rel", "importance"):
        assert torch.equal(fresh[k], case[k]), k
    got, traces, g = R.loss(case, torch.float64, grads=True)
    got32, traces32 = R.loss(case, torch.float32)
    for k in got:
        assert abs(float(ref[k + ".f64"]) - float(got[k])) <= 1e-12 * max(1.0, abs(float(got[k]))), k
        # the recorded fp32 run of the reference is an fp32 evaluation of the same value
        assert abs(float(ref[k + ".f32"]) - float(got[k])) <= 1e-4 * float(ref[k + ".mag"]), k
        assert float(ref[k + ".mag"]) >= abs(float(got[k]))
    for k in g:
        assert float((torch.from_numpy(ref["grad.%s.f64" % k]) - g[k]).abs().max()) <= 1e-12
        assert ref["grad.%s.f32" % k].dtype == np.float32
    for b, (tr, tr32) in enumerate(zip(traces, traces32)):
        for k in ("box_rows", "box_cols", "triplet_rows", "triplet_cols", "query_of_gt"):
            assert np.array_equal(ref["%s.%d" % (k, b)], tr[k]), (k, b)
            assert np.array_equal(tr[k], tr32[k]), (k, b)
        assert R.margin(tr["box_cost"].numpy()) > 1e-3
        assert R.margin(tr["id_cost"].numpy()) > 1e-3


# ---------------------------------------------------------------------- (3) the cost statement
def test_cost_terms_is_the_assigners_cost_and_its_magnitude_dominates():
    case = R.make_case(seed=9, G=(6, 1), T=(4, 1), planted=False,
                       shapes=[(50, 61), (64, 80)])
    case["gt_rels"][1] = torch.tensor([[0, 0, 1]])
    assigner = R.build_parts(case["num_classes"], case["num_relations"])[0]
    for b in range(2):
        h, w = case["img_metas"][b]["img_shape"][:2]
        f = torch.tensor([w, h, w, h], dtype=torch.float32)
        cost, mag = R.cost_terms(case["cls"][b], case["bbox"][b], case["gt_labels"][b],
                                 case["gt_bboxes"][b], f)
        ref = assigner.cost(case["bbox"][b].double(), case["cls"][b].double(),
                            case["gt_bboxes"][b].double(), case["gt_labels"][b],
                            case["img_metas"][b])
        assert cost.dtype == torch.float64 and float((cost - ref).abs().max()) <= 1e-12
        assert bool((mag >= cost.abs()).all()) and bool(torch.isfinite(mag).all())
        # fp32 evaluation of the same statement: a few units of 2^-24 mag
        c32, _ = R.cost_terms(case["cls"][b], case["bbox"][b], case["gt_labels"][b],
                              case["gt_bboxes"][b], f, dtype=torch.float32)
        assert float(((c32.double() - cost).abs() / mag).max()) <= 64 * 2.0 ** -24


def test_giou_edge_cases():
    b = torch.tensor([[10.0, 10.0, 20.0, 30.0]], dtype=torch.float64)
    g = lambda a, c: float(R.giou_parts(a, c)[0])
    assert g(b, b) == 1.0                                                 # equal boxes
    far = torch.tensor([[40.0, 50.0, 50.0, 60.0]], dtype=torch.float64)
    assert -1.0 < g(b, far) < 0.0                                         # disjoint
    inner = torch.tensor([[12.0, 12.0, 15.0, 15.0]], dtype=torch.float64)
    assert abs(g(b, inner) - 9.0 / 200.0) < 1e-15                         # enclosed: GIoU = IoU
    dot = torch.tensor([[15.0, 15.0, 15.0, 15.0]], dtype=torch.float64)
    assert g(dot, dot) == 0.0                                             # both clamps: 0 / eps - 0
    assert g(b, dot) == 0.0                                               # a zero-area box inside


# ------------------------------------------------------------ (4) ABI, refusals, configuration
def test_header_binding_sources_and_exports_declare_the_new_entry():
    import pairnet_amd
    from pairnet_amd import hip
    from pairnet_amd import build as B
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    name = "pn_box_match_cost_f32"
    assert name in declared and name in hip._SIGS and name in hip.EXPORTS
    assert "box_loss" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "box_loss.hip"))
    for cite in ("pairnet_bbox_head.py:863-865", "cross_r101_vg.py:158-163"):
        assert cite in header, cite
    assert callable(pairnet_amd.CrossHeadBBox.loss) and callable(pairnet_amd.CrossHeadBBox.val_losses)


def test_bad_arguments_are_refused_without_launching(built_lib):
    from pairnet_amd import hip
    lib = hip.lib()
    N, p = None, 1 << 20
    ok = [p, p, p, 3, p, 3, p, p, p, 300, 300, 1, 100, 150, 2.0, 5.0, 2.0, 0.25, 2.0, 1e-12, 1e-6, N]
    for i, v in ((0, N), (1, N), (2, N), (4, N), (6, N), (7, N), (8, N), (3, 0), (5, 0), (9, 0),
                 (10, 0), (10, 1024 * 1024 + 1), (11, 0), (12, 1), (12, 1025), (13, 0), (13, 257)):
        args = list(ok)
        args[i] = v
        assert lib.pn_box_match_cost_f32(*args) == -1, i


def test_head_accepts_train_cfg_and_the_loss_refuses_what_it_does_not_cover():
    from pairnet_amd import CrossHeadBBox
    from pairnet_amd.bbox_losses import CrossHeadBBoxLoss
    from pairnet_amd.config import bbox_head_cfg
    cfg = bbox_head_cfg()
    cfg.pop("type", None)
    tc = dict(id_assigner=dict(type="IdMatcher", sub_id_cost=dict(type="ClassificationCost", weight=1.0),
                               obj_id_cost=dict(type="ClassificationCost", weight=1.0),
                               r_cls_cost=dict(type="ClassificationCost", weight=0.0)),
              bbox_assigner=dict(type="HungarianAssigner",
                                 cls_cost=dict(type="FocalLossCost", weight=2.0),
                                 reg_cost=dict(type="BBoxL1Cost", weight=5.0, box_format="xywh"),
                                 iou_cost=dict(type="IoUCost", iou_mode="giou", weight=2.0)),
              sampler=dict(type="PseudoSampler"))
    cfg["train_cfg"] = tc
    head = CrossHeadBBox(**cfg)
    assert head.train_cfg == tc
    loss = CrossHeadBBoxLoss(150, 50, 100, train_cfg=tc)
    assert loss.Q == 100 and loss.box_w == (2.0, 5.0, 2.0)
    import copy
    for path, value in ((("bbox_assigner", "type"), "MaskHungarianAssigner"),
                        (("bbox_assigner", "cls_cost", "type"), "ClassificationCost"),
                        (("bbox_assigner", "reg_cost", "box_format"), "xyxy"),
                        (("bbox_assigner", "iou_cost", "iou_mode"), "iou"),
                        (("sampler", "type"), "MaskPseudoSampler"),
                        (("id_assigner", "type"), "OldIdMatcher")):
        bad = copy.deepcopy(tc)
        d = bad
        for k in path[:-1]:
            d = d[k]
        d[path[-1]] = value
        with pytest.raises(NotImplementedError):
            CrossHeadBBoxLoss(150, 50, 100, train_cfg=bad)
    with pytest.raises(NotImplementedError):
        CrossHeadBBoxLoss(150, 50, 100, train_cfg=tc, rel_cls_loss=dict(type="MultilabelFocalLoss"))
