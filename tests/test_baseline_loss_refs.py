"""CPU: (1) the float64 statement of tests/baseline_loss_ref.py equals, to 1e-12, the reference's OWN
`CrossHeadBaseline.loss` (all 30 terms and the three relation-logit gradients), executed in place
under name-only stubs where the reference tree is present, and the fixture
tests/golden/baseline_loss.npz holds what that loss computes in fp32; (2) the planted conditions of
the GPU cases hold: every id assignment leads by more than twice the cost kernel's bound, and the
fp32 and float64 runs agree on it; (3) the C ABI declares the new entries, bad arguments and option
sets are refused without a launch, and csrc/rel_loss.hip compiles for gfx950 without scratch.  The
kernels run in tests/test_baseline_loss_gpu.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import baseline_loss_ref as BR
import loss_optim_ref as R
import seg_loss_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle import ref_shim  # noqa: E402

NEW = ("pn_rel_id_cost_f32", "pn_rel_targets", "pn_id_ce_f32")
need_ref = pytest.mark.skipif(not ref_shim.available(), reason="reference tree absent")


# ---------------------------------------------------------------- (1) the statement is pinned
@need_ref
@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_equals_the_references_own_loss_in_float64(name):
    case, _ = BR.golden_case(name)
    out, (g_rel, g_sub, g_obj), g_cls = BR.run_reference(case, torch.float64)
    seg, r = BR.run_whole(case)
    L = case["cls"].shape[0]
    want = dict(seg["losses"], **r["losses"])
    assert set(out) == set(want) and len(out) == 3 * L + 3
    for k in out:
        assert abs(float(out[k]) - float(want[k])) <= 1e-12, k
    for got, ref in ((g_rel, r["g_rel"]), (g_sub, r["g_sub"]), (g_obj, r["g_obj"]), (g_cls, seg["g_cls"])):
        assert float((got - ref).abs().max()) <= 1e-12
    assert name != "b" or float(r["g_sub"][0].abs().max()) == 0.0      # one matched column: exactly 0


@need_ref
def test_fixture_holds_what_the_reference_computes_in_fp32():
    for name in ("a", "b"):
        case, ref = BR.golden_case(name)
        out, grads, _ = BR.run_reference(case, torch.float32)
        got = np.array([float(out[k]) for k in ref["names"]], np.float32)
        assert np.array_equal(got, ref["loss32"])
        for key, g in zip(("g_rel32", "g_sub32", "g_obj32"), grads):
            assert np.array_equal(g.numpy(), ref[key]), key


def test_fixture_holds_the_restatements_float64_values():
    for name in ("a", "b"):
        case, ref = BR.golden_case(name)
        seg, r = BR.run_whole(case)
        v64 = dict(seg["losses"], **r["losses"])
        assert len(ref["names"]) == 30 - 27 + 3 * case["cls"].shape[0]
        for k, v in zip(ref["names"], ref["loss64"]):
            assert abs(float(v64[str(k)]) - v) <= 1e-12
        assert np.array_equal(seg["matched"].numpy(), ref["matched"])
        assert np.array_equal(r["pos"].numpy(), ref["pos"])
        assert np.array_equal(r["r_labels"].numpy(), ref["r_labels"])
        for b in range(case["cls"].shape[1]):
            assert np.array_equal(np.stack(r["pairs"][b]), ref["pairs.%d" % b])
        for key in ("g_rel", "g_sub", "g_obj"):
            scale = S.U * r[key + "_mag"].numpy() + S.FLT_MIN
            assert (np.abs(ref[key + "32"] - r[key].numpy()) <= (float(ref[key + "_ratio"]) + 1e-6) * scale).all()
        err = np.abs(ref["loss32"].astype(np.float64) - ref["loss64"])
        assert (err <= (ref["loss_ratio"] + 1e-6) * S.U * ref["loss_mag"] + S.FLT_MIN).all()


def test_pieces_equal_torch_and_the_oracle():
    from oracle.mmdet_train import ClassificationCost
    c = BR.scores_case(1, 8, 8, 6, (4,), (5,), seed=3)
    a = BR.assigned_queries(4, *c["od"][0])
    gr = c["gt_rels"][0]
    cost, mag = BR.id_cost(c["rel"][0], c["sub"][0], c["obj"][0], gr, a)
    cc = ClassificationCost(weight=1.0)
    want = cc(c["sub"][0].double(), a[gr[:, 0]]) + cc(c["obj"][0].double(), a[gr[:, 1]]) + \
        cc(c["rel"][0].double(), gr[:, 2])
    assert float((cost - want).abs().max()) <= 1e-12 and bool((mag >= cost.abs() - 1e-15).all())
    # the fill of an object without a query is 1 (baseline.py:829), not -1
    assert BR.assigned_queries(3, torch.tensor([5]), torch.tensor([2])).tolist() == [1, 1, 5]
    rows, cols, tgt = np.array([1, 4, 6]), torch.tensor([0, 3, 5, 7]), torch.tensor([2, 0, 3])
    v, m, lo = BR.id_ce(c["sub"][0], rows, cols, tgt, 2.0, 2)
    f = c["sub"][0].double()[rows][:, cols]
    want = 2.0 * torch.nn.functional.cross_entropy(f, tgt) / 2
    assert abs(float(v) - float(want)) <= 1e-12 and float(m) >= abs(float(v)) and lo > 0


# ---------------------------------------------------------------- (2) planted conditions
def _relation_cases():
    """Every case whose id assignment a GPU test compares: (name, relation inputs, od, G, planted)."""
    for name in ("a", "b"):
        case, _ = BR.golden_case(name)
        seg = S.run_whole(case, grad=False)
        L, B = case["cls"].shape[:2]
        od, G = BR.od_of(seg["matched"], L, B, case["gt_labels"])
        yield "fixture " + name, case, od, G, None
    for shape in BR.COST_SHAPES:
        for B in (1, 2, 3):
            c = BR.cost_case(*shape, B)
            yield "cost %s B %d" % (shape, B), c, c["od"], c["G"], c["planted"]
    for name in BR.ID_CASES:
        c = BR.id_case(name)
        yield "id " + name, c, c["od"], c["G"], c["planted"]


def test_every_id_assignment_case_leads_by_more_than_the_cost_bound():
    n = 0
    for name, c, od, G, planted in _relation_cases():
        r = BR.relation_loss(c["rel"], c["sub"], c["obj"], c["gt_rels"], od, G, c["rel_class_weight"],
                             grad=False)
        r32 = BR.relation_loss(c["rel"], c["sub"], c["obj"], c["gt_rels"], od, G,
                               c["rel_class_weight"], dtype=torch.float32, grad=False)
        Bn, Rn, C1 = c["rel"].shape
        Q = c["sub"].shape[-1]
        for b in range(Bn):
            rows, cols = r["pairs"][b]
            # the fp32 and float64 runs agree on the assignment
            assert np.array_equal(rows, r32["pairs"][b][0]) and np.array_equal(cols, r32["pairs"][b][1]), (name, b)
            Gr = c["gt_rels"][b].shape[0]
            if planted is not None and Gr <= Rn:
                assert sorted(zip(rows.tolist(), cols.tolist())) == planted[b], (name, b)
            cost = r["costs"][b]
            margin = R.assignment_margin(cost, rows, cols)
            # the cost kernel's rounding count (with the largest z, 88) x 2^-24 x 3 (three softmax
            # entries <= 1, unit weights) plus twice the torch fp32 oracle's own error
            a = 2.0 * float((r32["costs"][b].double() - cost).abs().max())
            bound = (BR.cost_chain(Q, C1) + 88 + 4) * S.U * 3.0 + a
            assert 2 * bound < margin.min(), (name, b, bound, margin.min())
            n += 1
    assert n >= 2 * 2 + 5 * 6 + 8


# ---------------------------------------------------------------- (3) ABI, refusals, compile
def test_header_binding_sources_and_exports_declare_the_new_entries():
    import pairnet_amd
    from pairnet_amd import api, hip
    from pairnet_amd import build as B
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in hip._SIGS and name in hip.EXPORTS, name
    assert "rel_loss" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "rel_loss.hip"))
    for fn in ("rel_id_cost", "rel_targets", "id_ce"):
        assert callable(getattr(hip, fn)), fn
    for cite in ("baseline.py:655-694, 828-907", "approaches/matcher.py:323-330", "baseline.py:866-907",
                 "losses/seg_losses.py:47-57", "baseline_r50_psg.py:336-350"):
        assert cite in header, cite
    assert "BaselineRelationLoss" in api.__all__ and hasattr(pairnet_amd, "BaselineRelationLoss")
    assert callable(pairnet_amd.CrossHeadBaseline.full_losses) and callable(pairnet_amd.PSGTr.val_full_losses)


def test_bad_arguments_are_refused_without_launching(built_lib):
    from pairnet_amd import hip
    lib = hip.lib()
    N, p = None, 1 << 20
    ok = [p, p, p, p, 4, p, 3, p, p, 24, 1, 8, 8, 6, 1.0, 1.0, 1.0, N]
    for i, v in ((0, N), (3, N), (7, N), (8, N), (4, 0), (6, 0), (9, 0), (10, 0), (11, 1025), (12, 1025),
                 (13, 0)):
        args = list(ok)
        args[i] = v
        assert lib.pn_rel_id_cost_f32(*args) == -1, i
    ok = [p, p, p, 3, p, p, 4, p, 3, 1, 8, 8, 6, p, p, p, N]
    for i, v in ((0, N), (1, N), (4, N), (13, N), (14, N), (15, N), (3, 0), (6, 0), (8, 0), (9, 0), (10, 1025),
                 (11, 0), (12, 0)):
        args = list(ok)
        args[i] = v
        assert lib.pn_rel_targets(*args) == -1, i
    ok = [p, p, p, 3, p, p, 3, 1, 8, 8, 2.0, 2.0, p, p, p, p, N]
    for i, v in ((0, N), (2, N), (4, N), (5, N), (12, N), (13, N), (14, N), (3, 0), (6, 0), (7, 0), (8, 1025),
                 (9, 0)):
        args = list(ok)
        args[i] = v
        assert lib.pn_id_ce_f32(*args) == -1, i


def _cpu_call(obj, c, **over):
    kw = dict(rel=c["rel"], sub=c["sub"], obj=c["obj"], gt_rels=c["gt_rels"],
              matched=BR.matched_rows(c["od"], c["G"]), num_gts=c["G"])
    kw.update(over)
    return obj.loss(kw["rel"], kw["sub"], kw["obj"], kw["gt_rels"], kw["matched"], kw["rel"].shape[0],
                    num_gts=kw["num_gts"])


def test_the_loss_object_refuses_from_shapes_before_any_launch():
    """Host tensors throughout, on a machine without a GPU: nothing can have been launched."""
    from pairnet_amd import BaselineRelationLoss
    c = BR.scores_case(2, 8, 8, 6, (3, 4), (2, 3), seed=5)
    obj = BaselineRelationLoss(5, 8, 8)
    with pytest.raises(ValueError, match="no ground-truth relation"):
        _cpu_call(obj, c, gt_rels=[c["gt_rels"][0], torch.zeros(0, 3, dtype=torch.int64)])
    with pytest.raises(ValueError, match="queries"):
        _cpu_call(obj, c, num_gts=[3, 9])
    bad = c["gt_rels"][1].clone()
    bad[0, 1] = 4
    with pytest.raises(ValueError, match="objects outside"):
        _cpu_call(obj, c, gt_rels=[c["gt_rels"][0], bad])
    for p in (0, 6):
        bad = c["gt_rels"][0].clone()
        bad[1, 2] = p
        with pytest.raises(ValueError, match="predicates outside"):
            _cpu_call(obj, c, gt_rels=[bad, c["gt_rels"][1]])
    with pytest.raises(ValueError):
        _cpu_call(obj, c, rel=c["rel"][:, :, :5])
    with pytest.raises(ValueError):
        _cpu_call(obj, c, matched=BR.matched_rows(c["od"], c["G"])[:-1])
    with pytest.raises(ValueError):
        _cpu_call(obj, c, num_gts=None)


def test_option_sets_outside_the_config_are_refused():
    from pairnet_amd import BaselineRelationLoss, CrossHeadBaseline
    from helpers import baseline_cfg
    BaselineRelationLoss(56, 100, 100)
    cc = dict(type="ClassificationCost", weight=1.0)
    old = dict(type="OldIdMatcher", sub_id_cost=cc, obj_id_cost=cc, r_cls_cost=cc)
    obj = BaselineRelationLoss(56, 100, 100, train_cfg=dict(id_assigner=dict(
        old, sub_id_cost=dict(cc, weight=0.5), r_cls_cost=dict(cc, weight=3.0))),
        rel_loss_cls=dict(type="CrossEntropyLoss", loss_weight=1.5, class_weight=[0.1] + [1.0] * 56),
        sub_id_loss=dict(type="MultilabelCrossEntropy", loss_weight=0.25))
    assert (obj.c_sub, obj.c_obj, obj.c_rel) == (0.5, 1.0, 3.0)         # the weights are honoured
    assert (obj.w_rel, obj.w_sub, obj.w_obj) == (1.5, 0.25, 2.0) and obj.class_weight[0] == 0.1
    for kw in (dict(rel_loss_cls=dict(type="SeesawLoss", num_classes=57, loss_weight=2.0)),
               dict(train_cfg=dict(id_assigner=dict(old, type="IdMatcher"))),
               dict(train_cfg=dict(id_assigner=dict(old, obj_id_cost=dict(type="FocalLossCost", weight=1.0)))),
               dict(sub_id_loss=dict(type="CrossEntropyLoss", loss_weight=2.0)),
               dict(obj_id_loss=dict(type="MultilabelLogRegression", loss_weight=2.0)),
               dict(rel_loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True)),
               dict(train_cfg=dict(num_points=12544))):
        with pytest.raises(NotImplementedError):
            BaselineRelationLoss(56, 100, 100, **kw)
    with pytest.raises(ValueError):
        BaselineRelationLoss(56, 100, 100, rel_loss_cls=dict(type="CrossEntropyLoss", class_weight=[1.0] * 56))
    with pytest.raises(NotImplementedError):
        BaselineRelationLoss(56, 2000, 2000)
    # the head keeps its three loss options and refuses before launching
    head = CrossHeadBaseline(**baseline_cfg())
    assert head._rel_loss_cfg["sub_id_loss"]["type"] == "MultilabelCrossEntropy"
    rel = torch.zeros(1, head.num_rel_query, head.num_relations + 1)
    with pytest.raises(ValueError, match="no ground-truth relation"):
        head.full_losses(dict(rel=rel), dict(), [torch.zeros(0, 3)], None, [torch.tensor([1])], [None], [{}])
    with pytest.raises(ValueError, match="queries"):
        head.full_losses(dict(rel=rel), dict(), [torch.tensor([[0, 0, 1]])], None,
                         [torch.zeros(head.num_obj_query + 1, dtype=torch.int64)], [None], [{}])


def test_rel_loss_kernels_compile_for_gfx950_without_scratch(tmp_path):
    from pairnet_amd import build as B
    out = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(B.CSRC, "rel_loss.hip"), "-o", str(tmp_path / "rel_loss.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+(.*)", line)
        if not m:
            continue
        f = re.match(r"Function Name: (\S+)", m.group(1))
        if f:
            cur = res.setdefault(f.group(1), {})
            continue
        kv = re.match(r"(.+?): (\d+)", m.group(1))
        if kv and cur is not None:
            cur[kv.group(1).strip()] = int(kv.group(2))
    for n in ("k_rel_id_cost", "k_rel_targets", "k_id_ce", "k_id_ce_finish"):
        hit = [k for k in res if n in k]
        assert hit, (n, sorted(res))
        for k in hit:
            assert res[k]["ScratchSize [bytes/lane]"] == 0, k
            assert res[k]["LDS Size [bytes/block]"] <= 9 * 1024, k
