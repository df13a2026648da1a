"""No GPU: what PSGTrHead2's loss tests stand on (tests/tri_loss_ref.py).

  (1) the float64 statement of the cost equals `oracle.mmdet_train`'s three cost classes summed as
      `MaskHTriMatcher.assign` sums them, and the class terms equal torch's `F.cross_entropy` under
      mmdet's reduction (1e-12);
  (2) the statement of the whole loss equals the reference's own `PSGTrHead2.loss` with its own
      `MaskHTriMatcher`, run in place through oracle/ref_shim: values and autograd gradients to
      1e-10, identical assigned pairs (skipped where the reference tree is absent);
  (3) every planted case has a margin: the cheapest total with any one planted pair forbidden is at
      least 0.5 cost units above the optimum, and the optimum IS the planted assignment;
  (4) the fixture tests/golden/tri_loss.npz holds what the builder and the statement give today;
  (5) the new entries are declared, bound, built and refuse bad arguments without launching; the ABI
      is still 34;
  (6) the constructor's refusals, the ValueErrors and the label fills (the relation fill at
      `num_relations` with the 0.02 at index 0).
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tri_loss_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = dict(T.CASES, **{"golden_" + k: v for k, v in T.GOLDEN_CASES.items()})


def _ref_available():
    from oracle import ref_shim
    return ref_shim.available()


needs_reference = pytest.mark.skipif(not _ref_available(), reason="reference tree absent")


# ------------------------------------------------------------------- (1) pinned to torch / mmdet
@pytest.mark.parametrize("name", ["small", "sat"])
def test_cost_statement_equals_the_mmdet_costs_summed_in_the_matchers_order(name):
    from oracle import mmdet_train as M
    case = T.tri_case(**T.CASES[name])
    w = T.CFG["cost"]
    costs = [M.ClassificationCost(w[0]), M.CrossEntropyLossCost(w[1]), M.DiceCost(w[2], True, 1.0),
             M.ClassificationCost(w[3]), M.CrossEntropyLossCost(w[4]), M.DiceCost(w[5], True, 1.0),
             M.ClassificationCost(w[6])]
    real_float = torch.Tensor.float
    for b in range(2):
        r = T.image_cost(case, b)
        xs, xo, t = T.image_samples(case, b)
        gr, gl = case["gt_rels"][b], case["gt_labels"][b]
        args = [(case["sub"][0, b].double(), gl[gr[:, 0]]), (xs, t[gr[:, 0]]), (xs, t[gr[:, 0]]),
                (case["obj"][0, b].double(), gl[gr[:, 1]]), (xo, t[gr[:, 1]]), (xo, t[gr[:, 1]]),
                (case["rel"][0, b].double(), gr[:, 2])]
        torch.Tensor.float = lambda self, *a, **k: self.double()     # (the costs' `.float()` casts)
        try:
            terms = [c(*a) for c, a in zip(costs, args)]
        finally:
            torch.Tensor.float = real_float
        want = terms[0]
        for term in terms[1:]:
            want = want + term
        assert want.dtype == torch.float64 and tuple(want.shape) == (8, gr.shape[0])
        # (1e-12 of the cell's magnitude: at +-80 logits the two float64 forms of the mask term,
        # pos @ t + neg @ (1 - t) there and neg - x @ t here, round magnitudes of several hundred)
        assert bool(((r["cost"] - want).abs() <= 1e-12 * (1.0 + r["mag"])).all())
        assert name == "sat" or float((r["cost"] - want).abs().max()) <= 1e-12
        assert bool((r["mag"] >= r["cost"].abs() - 1e-12).all())
        r32 = T.image_cost(case, b, torch.float32)
        assert r32["cost"].dtype == torch.float32
        assert float((r32["cost"].double() - r["cost"]).abs().max()) <= 1e-3


def test_class_terms_equal_torch_cross_entropy_under_mmdets_reduction():
    case = T.tri_case(**T.CASES["small"])
    r = T.whole_loss(case, grad=False)
    B, Q = case["sub"].shape[1:3]
    cw_so, cw_r = T.class_weights(case["num_classes"], case["num_relations"])
    for i, (key, name, cw) in enumerate((("sub", "s_loss_cls", cw_so), ("obj", "o_loss_cls", cw_so),
                                         ("rel", "r_loss_cls", cw_r))):
        x, y = case[key].double().view(B * Q, -1), r["labels"][i]
        el = F.cross_entropy(x, y, weight=cw.double(), reduction="none")
        want = T.CFG["w_cls"][i] * el.sum() / (cw.double()[y].sum() + T.EPS32)
        assert abs(float(r["losses"][name]) - float(want)) <= 1e-12, name


# ------------------------------------------------------------------- (2) pinned to the reference
@needs_reference
@pytest.mark.parametrize("name", ["small", "r_gt_q", "sat"])
def test_statement_equals_the_references_own_loss_and_matcher(name):
    case = T.tri_case(**T.CASES[name])
    r = T.whole_loss(case)
    out, grads, pairs = T.run_reference(case, torch.float64)
    B, Q = case["sub"].shape[1:3]
    h, w = case["sub_seg"].shape[-2:]
    assert set(out) == set(T.NAMES)
    mine = list(zip(r["matched"][:, 0].tolist(), r["matched"][:, 1].tolist(), r["rel_idx"].tolist()))
    assert mine == [(b, q, k) for b in range(B) for q, k in pairs[b]]       # identical assigned pairs
    for k in T.NAMES:
        assert abs(float(out[k]) - float(r["losses"][k])) <= 1e-10, k
    for k in ("sub", "obj", "rel"):
        assert float((grads[k] - r["g_" + k]).abs().max()) <= 1e-10, k
    for s, k in enumerate(("sub_seg", "obj_seg")):
        g = grads[k].reshape(B * Q, h, w)
        assert float((g[r["mask_rows"]] - r["sides"][s]["g_mask"]).abs().max()) <= 1e-10, k
        other = torch.ones(B * Q, dtype=torch.bool)
        other[r["mask_rows"]] = False
        assert float(g[other].abs().max()) == 0.0


# ------------------------------------------------------------------- (3) the margin condition
@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_planted_assignment_has_a_margin_of_half_a_cost_unit(name):
    case = T.tri_case(**ALL_CASES[name])
    for b in range(case["sub"].shape[1]):
        r = T.image_cost(case, b)
        m, pairs = T.margin(r["cost"], case["planted"][b])
        print("%s image %d: margin %.3f" % (name, b, m))
        assert pairs == case["planted"][b]
        assert m >= 0.5, (name, b, m)
        # the torch-fp32 statement assigns alike
        r32 = T.image_cost(case, b, torch.float32)
        assert T.margin(r32["cost"], case["planted"][b])[1] == pairs


def test_the_named_shapes_hold_what_they_are_named_for():
    small = T.tri_case(**T.CASES["small"])
    gr = small["gt_rels"][0]
    assert gr[0, :2].tolist() == gr[1, :2].tolist() and int(gr[0, 2]) != int(gr[1, 2])   # two predicates
    assert bool((gr[:, 0] == gr[:, 1]).any())                                           # a self-relation
    assert 3 not in gr[:, :2].reshape(-1).tolist()                      # an object no relation names
    assert int(small["gt_masks"][0][0].sum()) == 0                                      # an all-zero mask
    assert len({tuple(r) for r in gr.tolist()}) == gr.shape[0]
    more = T.tri_case(**T.CASES["r_gt_q"])
    assert more["gt_rels"][0].shape[0] > more["sub"].shape[2] and more["gt_rels"][1].shape[0] == 1
    wide = T.CASES["wide"]
    assert wide["G"][0] > 8 and wide["Np"] > 256 and wide["Q"] > 64
    groups = T.tri_case(**T.CASES["groups"])
    assert groups["gt_labels"][0].shape[0] > 16 and int(groups["gt_rels"][0][:, :2].max()) >= 16
    sat = T.tri_case(**T.CASES["sat"])
    assert bool((sat["gt_masks"][0][1] == 1).all()) and float(sat["sub_seg"].abs().max()) == 80.0
    assert 1 in sat["gt_rels"][0][:, :2].reshape(-1).tolist()


# ------------------------------------------------------------------- (4) the fixture
@pytest.mark.parametrize("name", ["a", "b"])
def test_fixture_holds_what_the_builder_and_the_statement_give(name):
    case, ref = T.golden_case(name)
    built = T.tri_case(**T.GOLDEN_CASES[name])
    for k in T._TENSORS:
        assert torch.equal(case[k], built[k]), k
    for b in range(2):
        for k in ("gt_labels", "gt_masks", "gt_rels"):
            assert torch.equal(case[k][b], built[k][b]), k
        assert torch.equal(case["points"]["assign"][b], built["points"]["assign"][b])
    for k in T._POINTS:
        assert torch.equal(case["points"][k], built["points"][k]), k
    r = T.whole_loss(case)
    assert np.array_equal(ref["matched"], r["matched"].numpy())
    assert np.array_equal(ref["rel_idx"], r["rel_idx"].numpy())
    assert list(ref["names"]) == list(T.NAMES)
    for i, k in enumerate(T.NAMES):
        assert abs(float(ref["loss64"][i]) - float(r["losses"][k])) <= 1e-12, k
        assert abs(float(ref["loss_mag"][i]) - float(r["mags"][k])) <= 1e-12, k
        # the reference's own fp32 run sits within a few roundings of the float64 value
        assert float(ref["loss_ratio"][i]) < 64, k
    for k in ("g_sub", "g_obj", "g_rel", "g_sub_mask", "g_obj_mask"):
        assert ref[k + "32"].dtype == np.float32 and float(ref[k + "_ratio"]) < 64, k
    assert os.path.getsize(T.GOLDEN) < 1 << 20


# ------------------------------------------------------------------- (5) ABI and refusals
def test_header_binding_sources_and_exports_declare_the_new_entries():
    import pairnet_amd
    from pairnet_amd import api, hip
    from pairnet_amd import build as B
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    tri = sorted(n for n in declared if n.startswith("pn_tri_"))
    assert tri == ["pn_tri_match_cost_f32", "pn_tri_pair_splits", "pn_tri_targets"]
    for name in tri:
        assert name in hip._SIGS and name in hip.EXPORTS, name
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION == 34
    assert "tri_loss" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "tri_loss.hip"))
    for cite in ("psgtr_head2.py:879-1018", "matcher.py:29-102", "psgtr_r50_psg_plus.py:162-177",
                 "psgtr_head2.py:967-997"):
        assert cite in header, cite
    assert callable(hip.tri_match_cost) and callable(hip.tri_targets)
    sites = (hip.TRI_SITE_ASSIGN, hip.TRI_SITE_SUB_CANDIDATES, hip.TRI_SITE_SUB_TAIL,
             hip.TRI_SITE_OBJ_CANDIDATES, hip.TRI_SITE_OBJ_TAIL)
    assert len(set(sites)) == 5 and min(sites) >= 4 * 64     # clear of seg_losses.py's 4 * layer + k
    assert "PSGTrHead2Loss" in api.__all__ and "psgtr2_train_cfg" in api.__all__
    assert callable(pairnet_amd.PSGTrHead2.triplet_losses) and callable(pairnet_amd.PSGTr.val_triplet_losses)
    src = open(os.path.join(B.CSRC, "tri_loss.hip")).read()
    assert "atomicAdd" not in src and "float atomics" not in src.replace("no floating-point atomics", "")


def test_bad_arguments_are_refused_without_launching(built_lib):
    from pairnet_amd import hip
    lib = hip.lib()
    N, p = None, 1 << 20
    ns = lib.pn_tri_pair_splits(2, 8, 50)
    assert ns == 1 and lib.pn_tri_pair_splits(2, 100, 12544) == 5 and lib.pn_tri_pair_splits(0, 8, 50) == 0
    assert lib.pn_tri_pair_splits(1, 4, 1 << 20) == 16 and lib.pn_tri_pair_splits(64, 64, 300) == 1
    ok = [p] * 8 + [8, p, 7, p, 2, 8, 6, 5, 13, 21, 13, 21, 50, 4, 40, p, p, p, p, p, p,
                    4 * (7 + 2) * 8 * ns, p, 64, N]
    for i, v in [(k, N) for k in (0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 23, 24, 25, 26, 27, 28, 30)] + \
            [(8, 0), (10, 0), (12, 0), (13, 0), (14, 1), (15, 1), (16, 0), (17, 0), (18, 0), (19, 0),
             (20, 0), (21, 0), (21, 8), (22, 0), (29, 4 * (7 + 2) * 8 * ns - 1), (31, 0), (6, p + 4)]:
        args = list(ok)
        args[i] = v
        assert lib.pn_tri_match_cost_f32(*args) == -1, i
    ok = [p, p, p, 8, p, p, 8, p, 7, 2, 8, 5, 4, 8, p, p, p, p, p, p, N]
    for i, v in [(k, N) for k in (0, 1, 2, 4, 5, 7, 14, 15, 16, 17, 18, 19)] + \
            [(3, 0), (6, 0), (8, 0), (9, 0), (10, 0), (11, 0), (12, 0), (13, 0)]:
        args = list(ok)
        args[i] = v
        assert lib.pn_tri_targets(*args) == -1, i


# ------------------------------------------------------------------- (6) refusals, errors, fills
def _kw(**over):
    from pairnet_amd import psgtr2_head_cfg, psgtr2_train_cfg
    cfg = psgtr2_head_cfg()
    kw = {k: cfg[k] for k in ("sub_loss_cls", "sub_loss_mask", "sub_loss_dice", "obj_loss_cls",
                              "obj_loss_mask", "obj_loss_dice", "rel_loss_cls")}
    kw["train_cfg"] = psgtr2_train_cfg()
    for path, v in over.items():
        d, keys = kw, path.split("__")
        for k in keys[:-1]:
            d[k] = dict(d[k])
            d = d[k]
        d[keys[-1]] = v
    return kw


def test_constructor_takes_the_config_and_refuses_what_is_not_built():
    from pairnet_amd import PSGTrHead2Loss
    obj = PSGTrHead2Loss(133, 56, 100, **_kw())
    dflt = PSGTrHead2Loss(133, 56, 100)
    assert obj.cost_weights == dflt.cost_weights == [2.0, 5.0, 5.0, 2.0, 5.0, 5.0, 2.0, 1.0, 1.0]
    assert obj.w_cls == (1.0, 1.0, 2.0) and obj.w_mask == (5.0, 5.0) and obj.w_dice == (5.0, 5.0)
    assert obj.num_points == 12544 and obj.assign_status is None and obj.last is None
    for over in (dict(train_cfg__assigner__type="HTriMatcher"),
                 dict(train_cfg__assigner__s_mask_cost__type="BBoxL1Cost"),
                 dict(train_cfg__assigner__o_dice_cost__pred_act=False),
                 dict(train_cfg__assigner__r_cls_cost__type="FocalLossCost"),
                 dict(train_cfg__sampler__type="PseudoSampler"),
                 dict(sub_loss_cls__type="FocalLoss"), dict(rel_loss_cls__use_sigmoid=True),
                 dict(obj_loss_mask__use_sigmoid=False), dict(sub_loss_dice__naive_dice=False),
                 dict(obj_loss_dice__type="CrossEntropyLoss"), dict(sub_loss_mask__reduction="sum"),
                 dict(sub_loss_cls__class_weight=[1.0] * 134), dict(rel_loss_cls__class_weight=1),
                 dict(obj_loss_cls__class_weight=2.0)):
        with pytest.raises(NotImplementedError, match="built|float"):
            PSGTrHead2Loss(133, 56, 100, **_kw(**over))
    with pytest.raises(NotImplementedError):
        PSGTrHead2Loss(133, 56, 100, train_cfg=dict(num_points=50))
    with pytest.raises(NotImplementedError):
        PSGTrHead2Loss(133, 56, 100, bg_cls_weight=1)
    with pytest.raises(ValueError):
        PSGTrHead2Loss(133, 56, 100, **_kw(train_cfg__oversample_ratio=0.5))


def test_label_fills_and_class_weights_keep_the_references_two_facts():
    from pairnet_amd import PSGTrHead2Loss
    obj = PSGTrHead2Loss(5, 4, 8)
    assert obj.sub_class_weight == obj.obj_class_weight == [1.0] * 5 + [0.02]     # background LAST
    assert obj.rel_class_weight == [0.02] + [1.0] * 4                               # ... FIRST
    so, r = T.class_weights(5, 4)
    assert torch.equal(so, torch.tensor(obj.sub_class_weight)) and torch.equal(r, torch.tensor(obj.rel_class_weight))
    case = T.tri_case(**T.CASES["small"])
    res = T.whole_loss(case, grad=False)
    lab = res["labels"].view(3, 2, 8)
    planted = torch.zeros(2, 8, dtype=torch.bool)
    for b, pairs in case["planted"].items():
        for q, j in pairs:
            planted[b, q] = True
            so_, oo_, p_ = case["gt_rels"][b][j].tolist()
            assert lab[:, b, q].tolist() == [int(case["gt_labels"][b][so_]), int(case["gt_labels"][b][oo_]), p_]
    # unmatched queries: sub / obj at num_classes, rel at num_relations -- the LAST index, whose class
    # weight is class_weight (1.0), not the 0.02 that sits at index 0
    assert bool((lab[0][~planted] == 5).all()) and bool((lab[1][~planted] == 5).all())
    assert bool((lab[2][~planted] == 4).all())
    assert obj.rel_class_weight[4] == 1.0 and obj.rel_class_weight[0] == 0.02
    failed = T.targets([None, np.array([1, 4, 7])], [None, np.array([0, 1, 2])], case["gt_rels"],
                       case["gt_labels"], 8, 5, 4)
    assert bool((failed[1][:5] == -1).all()) and failed[1][5].tolist()[:2] == [1, 1]
    assert bool((failed[0][:, :8] == torch.tensor([[5], [5], [4]])).all())


def test_value_errors_come_before_anything_is_launched():
    from pairnet_amd import PSGTrHead2Loss
    case = T.tri_case(**T.CASES["small"])
    obj = PSGTrHead2Loss(5, 4, 8, train_cfg=T.train_cfg(50))
    cls = {k: case[k] for k in ("sub", "obj", "rel")}           # (host tensors: nothing can launch)
    seg = {k: case[k] for k in ("sub_seg", "obj_seg")}
    run = lambda rels, **kw: obj.loss(cls, seg, rels, None, case["gt_labels"], case["gt_masks"],
                                      [dict()] * 2, **kw)
    with pytest.raises(ValueError, match="image 1 has no ground-truth relation"):
        run([case["gt_rels"][0], torch.zeros(0, 3, dtype=torch.int64)])
    bad = case["gt_rels"][0].clone()
    bad[2, 1] = 4
    with pytest.raises(ValueError, match="objects outside"):
        run([bad, case["gt_rels"][1]])
    for v in (0, 5):
        bad = case["gt_rels"][1].clone()
        bad[0, 2] = v
        with pytest.raises(ValueError, match="predicates outside"):
            run([case["gt_rels"][0], bad])
    with pytest.raises(ValueError, match="unknown keys"):
        run(case["gt_rels"], points=dict(candidates=None))
    with pytest.raises(ValueError, match="fp32 logits"):
        obj.loss(dict(cls, rel=case["rel"][0]), seg, case["gt_rels"], None, case["gt_labels"],
                 case["gt_masks"], [dict()] * 2)
    with pytest.raises(AssertionError):
        run(case["gt_rels"], gt_bboxes_ignore=[None])


def test_head_keeps_the_loss_configs_and_the_detector_hands_train_cfg_down():
    from helpers import psgtr2_cfg
    from pairnet_amd import PSGTrHead2, build_detector, psgtr2_r50, psgtr2_train_cfg
    head = PSGTrHead2(**psgtr2_cfg())
    assert head._tri_loss is None and head.triplet_status() is None
    assert head._tri_loss_cfg["bg_cls_weight"] == 0.02 and head._tri_loss_cfg["train_cfg"] is None
    assert head._tri_loss_cfg["rel_loss_cls"]["loss_weight"] == 2.0
    model = psgtr2_r50()
    assert model["train_cfg"] == psgtr2_train_cfg()
    det = build_detector(model)
    assert det.bbox_head._tri_loss_cfg["train_cfg"] == psgtr2_train_cfg()
    # a config the loss does not cover still BUILDS (validated on first use)
    odd = PSGTrHead2(**dict(psgtr2_cfg(), sub_loss_cls=dict(type="FocalLoss")))
    with pytest.raises(NotImplementedError):
        odd.triplet_losses(dict(), dict(), [], None, [], [], [])
    off = PSGTrHead2(**dict(psgtr2_cfg(), use_mask=False))
    with pytest.raises(NotImplementedError, match="use_mask"):
        off.triplet_losses(dict(), dict(), [], None, [], [], [])
    for name in ("val_losses", "val_seg_losses", "val_full_losses", "trainer"):
        assert callable(getattr(det, name))
