"""GPU: the kernels of csrc/rel_loss.hip, the relation loss object (pair-net_amd/baseline_losses.py)
and the sibling head's full loss dict (`CrossHeadBaseline.full_losses`, `PSGTr.val_full_losses`)
against the float64 statement of tests/baseline_loss_ref.py and the fixture
tests/golden/baseline_loss.npz (recorded from the reference's own `CrossHeadBaseline.loss`).

Bound form (tests/test_seg_loss_gpu.py): |got - ref64| <= (c + a) * 2^-24 * mag + FLT_MIN per element.
`mag` is the float64 statement on absolute summands; `a` is twice the ratio the torch-fp32 run of the
same statement reaches against its float64 run, at least 4.  c, counted from the source (labnotes
R17.2; n the softmax length, z = min(88, max x - x[entry]) the subtraction in front of expf):

  k_rel_id_cost    z + ceil(n / 64) + ceil(ln n) + 13, n = max(Q, Cr + 1)   (baseline_loss_ref.cost_chain)
  k_id_ce value    ceil(ln n) + ceil(n / 64) + P + B + 14, n the matched columns, P the largest
                   number of positive rows of an image; the denominator's part is absolute in log d,
                   so every row's magnitude |m| + log d + |x_t| must be >= 1 (asserted)
  k_id_ce gradient z + ceil(ln n) + ceil(n / 64) + 13
  r_loss_cls       k_ce_avg / k_ce_avg_grad with L = 1, rows = B R (tests/test_seg_loss_gpu.py)"""
import math

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import baseline_loss_ref as BR
import seg_loss_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U, FLT_MIN = S.U, S.FLT_MIN
WORST = {}
_RUNS = {}


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
    assert not bool((err > c * U * mag + FLT_MIN).any()), (name, ratio, float(c.min()))
    return ratio


def _allow(v32, v64, mag):
    r = ((torch.as_tensor(v32).double() - torch.as_tensor(v64).double()).abs()
         / (U * torch.as_tensor(mag).double() + FLT_MIN))
    return max(4.0, 2.0 * float(r.max())) if r.numel() else 4.0


def _dev(t):
    return t.to(DEV).contiguous()


def _obj(c):
    from pairnet_amd import BaselineRelationLoss
    B, R, C1 = c["rel"].shape
    return BaselineRelationLoss(C1 - 1, c["sub"].shape[-1], R)


def _run_rel(key, c):
    """One run of the loss object on a scores_case (cached per case: the tests share it)."""
    if key not in _RUNS:
        assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
        obj, grads = _obj(c), {}
        out = obj.loss(_dev(c["rel"]), _dev(c["sub"]), _dev(c["obj"]), c["gt_rels"],
                       _dev(BR.matched_rows(c["od"], c["G"])), c["rel"].shape[0], grads=grads,
                       num_gts=c["G"])
        torch.cuda.synchronize()
        r = BR.relation_loss(c["rel"], c["sub"], c["obj"], c["gt_rels"], c["od"], c["G"],
                             c["rel_class_weight"])
        r32 = BR.relation_loss(c["rel"], c["sub"], c["obj"], c["gt_rels"], c["od"], c["G"],
                               c["rel_class_weight"], dtype=torch.float32)
        _RUNS[key] = (obj, out, grads, r, r32)
    return _RUNS[key]


def _blocks(obj, c):
    """The device's cost blocks and pairs per image, copied back."""
    R = c["rel"].shape[1]
    cost, rows, cols = obj.last["cost"].cpu(), obj.last["rows"].cpu().numpy(), obj.last["cols"].cpu().numpy()
    co = po = 0
    for b, gr in enumerate(c["gt_rels"]):
        Gr = gr.shape[0]
        P = min(R, Gr)
        yield b, cost[co:co + R * Gr].view(R, Gr), rows[po:po + P], cols[po:po + P]
        co, po = co + R * Gr, po + P


def _id_z(c, r, which):
    """z of every id gradient element: max over the row's matched columns minus the element."""
    x = c[which].double()
    z = torch.zeros_like(x)
    for b, row, _, _ in r["pos"].tolist():
        cols = c["od"][b][0].long()
        f = x[b, row, cols]
        z[b, row, cols] = (f.max() - f).clamp(max=88.0)
    return z


def _check_rel(name, c, obj, out, grads, r, r32, ref32=None):
    """The three values and the three gradients against float64 (and the reference's fp32)."""
    B, R, C1 = c["rel"].shape
    Q = c["sub"].shape[-1]
    n = max(len(od[0]) for od in c["od"])
    P = max(min(R, g.shape[0]) for g in c["gt_rels"])
    assert int(obj.assign_status.cpu()) == 0 and obj.last_on_device
    assert set(out) == set(BR.NAMES) and all(v.dim() == 0 and v.is_cuda for v in out.values())
    assert r["row_mag_min"] >= 1.0, r["row_mag_min"]                   # (the id chain's condition)
    chain = dict(r_loss_cls=math.ceil(C1 / 64) + 2 * B * R + 14 + math.ceil(math.log(C1) + 1),
                 loss_subject_match=BR.id_ce_chain(n, P, B), loss_object_match=BR.id_ce_chain(n, P, B))
    for k in BR.NAMES:
        ref, mag = float(r["losses"][k]), float(r["mags"][k])
        a = _allow(r32["losses"][k], ref, mag)
        _ratio("%s %s" % (name, k), out[k], ref, mag, chain[k] + a)
        WORST[k] = max(WORST.get(k, 0.0), WORST["%s %s" % (name, k)])
        if ref32 is not None:      # against the reference's own fp32 value: c plus its stored ratio
            i = list(ref32["names"]).index(k)
            assert abs(float(out[k]) - float(ref32["loss32"][i])) <= \
                (chain[k] + a + float(ref32["loss_ratio"][i])) * U * mag + FLT_MIN, (name, k)
    z = (c["rel"].double().amax(-1, keepdim=True) - c["rel"].double()).clamp(max=88.0)
    cs = dict(g_rel=B * R + math.ceil(C1 / 64) + 14 + z,
              g_sub=BR.id_grad_chain(n) + _id_z(c, r, "sub"), g_obj=BR.id_grad_chain(n) + _id_z(c, r, "obj"))
    for key, gk in (("g_rel", "rel"), ("g_sub", "subject_scores"), ("g_obj", "object_scores")):
        a = _allow(r32[key], r[key], r[key + "_mag"])
        _ratio("%s %s" % (name, key), grads[gk], r[key], r[key + "_mag"], cs[key] + a)
        WORST[key] = max(WORST.get(key, 0.0), WORST["%s %s" % (name, key)])
        if key != "g_rel":         # rows and columns outside the filter: exactly 0
            got = grads[gk].cpu()
            assert float(got[r[key + "_mag"] == 0].abs().max()) == 0.0, (name, key)
        if ref32 is not None:
            err = (grads[gk].cpu().double() - torch.from_numpy(ref32[key + "32"]).double()).abs()
            cc = cs[key] + a + float(ref32[key + "_ratio"])
            assert bool((err <= cc * U * r[key + "_mag"] + FLT_MIN).all()), (name, key)


# ------------------------------------------------------------------------------ cost and assignment
@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("shape", BR.COST_SHAPES)
def test_id_match_cost_against_float64(shape, B):
    c = BR.cost_case(*shape, B)
    obj, _, _, r, r32 = _run_rel(("cost", shape, B), c)
    assert float(c["rel"].abs().max()) > 60 and len({g.shape[0] for g in c["gt_rels"]}) == B
    chain = BR.cost_chain(shape[1], shape[2])
    for b, cost, _, _ in _blocks(obj, c):
        a = _allow(r32["costs"][b], r["costs"][b], r["cost_mags"][b])
        _ratio("k_rel_id_cost", cost, r["costs"][b], r["cost_mags"][b], chain + r["cost_z"][b] + a)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", BR.COST_SHAPES)
def test_id_assignment_equals_scipy_on_the_devices_own_cost(shape, B):
    c = BR.cost_case(*shape, B)
    obj, _, _, r, _ = _run_rel(("cost", shape, B), c)
    assert int(obj.assign_status.cpu()) == 0 and obj.last_on_device
    for b, cost, rows, cols in _blocks(obj, c):
        wr, wc = linear_sum_assignment(cost.numpy())
        assert np.array_equal(rows, wr) and np.array_equal(cols, wc), (shape, b)
        assert np.array_equal(rows, r["pairs"][b][0]) and np.array_equal(cols, r["pairs"][b][1])
        assert len(rows) == min(shape[0], c["gt_rels"][b].shape[0])
    assert torch.equal(obj.last["pos"].cpu().long(), r["pos"])
    assert torch.equal(obj.last["r_labels"].cpu(), r["r_labels"])


# ------------------------------------------------------------------------------ id cross entropy
@pytest.mark.parametrize("name", sorted(BR.ID_CASES))
def test_id_cross_entropy_values_and_gradients(name):
    from pairnet_amd import hip
    c = BR.id_case(name)
    obj, out, grads, r, r32 = _run_rel(("id", name), c)
    _check_rel("id " + name, c, obj, out, grads, r, r32)
    assert torch.equal(obj.last["pos"].cpu().long(), r["pos"])
    B, R, Q = c["sub"].shape
    if name == "only_one_column":      # one matched column: both terms and their gradients exactly 0
        assert float(out["loss_subject_match"]) == 0.0 and float(out["loss_object_match"]) == 0.0
        assert float(grads["subject_scores"].abs().max()) == 0.0
        assert float(grads["object_scores"].abs().max()) == 0.0
    if name == "one_column":
        n0 = min(R, c["gt_rels"][0].shape[0])
        assert float(obj.last["row_loss"][:n0].abs().max()) == 0.0
        assert float(grads["subject_scores"][0].abs().max()) == 0.0
        assert float(grads["object_scores"][0].abs().max()) == 0.0 and float(out["loss_subject_match"]) > 0
    if name == "all_columns":
        assert len(c["od"][0][0]) == Q
    if name == "one_row":
        assert all(g.shape[0] == 1 for g in c["gt_rels"]) and r["pos"].shape[0] == B
    # gradient buffers pre-filled with NaN come back fully written, with the same bits
    g1 = torch.full((B, R, Q), float("nan"), device=DEV)
    g2 = torch.full((B, R, Q), float("nan"), device=DEV)
    row_loss, o2 = torch.empty_like(obj.last["row_loss"]), torch.empty(2, device=DEV)
    hip.id_ce(_dev(c["sub"]), _dev(c["obj"]), obj.last["matched"], obj.last["tab"], obj.last["pos"],
              obj.w_sub, obj.w_obj, row_loss, o2, g1, g2)
    assert torch.equal(g1, grads["subject_scores"]) and torch.equal(g2, grads["object_scores"])
    assert torch.equal(o2[0], out["loss_subject_match"]) and torch.equal(o2[1], out["loss_object_match"])


# ------------------------------------------------------------------------------ the full loss
def _head(case):
    from pairnet_amd import CrossHeadBaseline, baseline_head_cfg
    Q = case["cls"].shape[2]
    cfg = baseline_head_cfg(num_obj_query=Q, num_rel_query=Q, num_classes=case["num_classes"],
                            num_relations=case["num_relations"])
    cfg.pop("type")
    cc = lambda w: dict(type="ClassificationCost", weight=w)
    tc = dict(id_assigner=dict(type="OldIdMatcher", sub_id_cost=cc(1.0), obj_id_cost=cc(1.0),
                               r_cls_cost=cc(1.0)),
              num_points=case["num_points"], oversample_ratio=3.0, importance_sample_ratio=0.75,
              mask_assigner=dict(type="MaskHungarianAssigner", cls_cost=cc(2.0),
                                 mask_cost=dict(type="CrossEntropyLossCost", weight=5.0, use_sigmoid=True),
                                 dice_cost=dict(type="DiceCost", weight=5.0, pred_act=True, eps=1.0)),
              sampler=dict(type="MaskPseudoSampler"))
    return CrossHeadBaseline(**cfg, train_cfg=tc)


def _full(head, case, **over):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    c = dict(case, **over)
    B = c["cls"].shape[1]
    grads = {}
    out = head.full_losses(dict(cls=_dev(c["cls"]), rel=_dev(c["rel"]), subject_scores=_dev(c["sub"]),
                                object_scores=_dev(c["obj"])), dict(mask=_dev(c["mask"])),
                           c["gt_rels"], None, c["gt_labels"], c["gt_masks"], [dict()] * B, grads=grads,
                           points=c["points"])
    torch.cuda.synchronize()
    return out, grads


@pytest.mark.parametrize("name", ["a", "b"])
def test_full_losses_on_the_fixture(name):
    case, ref32 = BR.golden_case(name)
    L, B, Q = case["cls"].shape[:3]
    assert (L, B, Q, tuple(case["mask"].shape[-2:]), case["num_points"]) == (2, 2, 8, (13, 21), 50)
    head = _head(case)
    out, grads = _full(head, case)
    seg, r = BR.run_whole(case)
    _, r32 = BR.run_whole(case, torch.float32)
    assert sorted(out) == sorted(str(k) for k in ref32["names"]) and len(out) == 3 * L + 3
    assert set(grads) == {"cls", "mask_rows", "mask", "rel", "subject_scores", "object_scores"}
    assert int(head.seg_status().cpu()) == 0 and int(head.rel_status().cpu()) == 0
    # the matched pairs are the reference's
    rel = head._rel_loss
    assert np.array_equal(head._seg_loss.last["matched"].cpu().numpy(), ref32["matched"])
    assert np.array_equal(rel.last["pos"].cpu().numpy(), ref32["pos"])
    assert np.array_equal(rel.last["r_labels"].cpu().numpy(), ref32["r_labels"])
    got = np.stack([rel.last["rows"].cpu().numpy(), rel.last["cols"].cpu().numpy()])
    assert np.array_equal(got, np.concatenate([ref32["pairs.%d" % b] for b in range(B)], 1))
    # the 27 segmentation terms and their three gradients: bitwise `seg_losses` alone
    g_seg = {}
    alone = head.seg_losses(dict(cls=_dev(case["cls"])), dict(mask=_dev(case["mask"])), case["gt_labels"],
                            case["gt_masks"], [dict()] * B, grads=g_seg, points=case["points"])
    assert len(alone) == 3 * L
    for k in alone:
        assert torch.equal(out[k], alone[k]), k
    for k in g_seg:
        assert torch.equal(grads[k], g_seg[k]), k
    # the three new terms and gradients within bound
    od, G = BR.od_of(seg["matched"], L, B, case["gt_labels"])
    c = dict(case, od=od, G=G)
    rel_out = {k: out[k] for k in BR.NAMES}
    _check_rel("fixture " + name, c, rel, rel_out, grads, r, r32, ref32)
    for i, k in enumerate(ref32["names"]):
        if str(k) in BR.NAMES:
            print("reference fp32 %s: ratio %.3f" % (k, float(ref32["loss_ratio"][i])))
    print("reference fp32 gradients:", {k: round(float(ref32[k + "_ratio"]), 3) for k in ("g_rel", "g_sub", "g_obj")})
    # a second call gives the same bits; so does a side stream
    out2, grads2 = _full(head, case)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out3, grads3 = _full(head, case)
    side.synchronize()
    for o, g in ((out2, grads2), (out3, grads3)):
        assert all(torch.equal(o[k], out[k]) for k in out)
        assert all(torch.equal(g[k], grads[k]) for k in grads)


# ------------------------------------------------------------------------------ status
def test_nan_in_one_images_rel_row_sets_the_status_and_leaves_the_rest_alone():
    case, ref32 = BR.golden_case("a")
    head = _head(case)
    clean, g_clean = _full(head, case)
    pos_clean = head._rel_loss.last["pos"].clone()
    row_clean = head._rel_loss.last["row_loss"].clone()
    assert int(head.rel_status().cpu()) == 0
    rel = case["rel"].clone()
    rel[1, 3, 2] = float("nan")
    out, grads = _full(head, case, rel=rel)
    st = int(head.rel_status().cpu())
    assert st == 1 and int(head.seg_status().cpu()) == 0           # pn_lsa_f32: a NaN entry
    n0 = min(8, case["gt_rels"][0].shape[0])
    pos, lab = head._rel_loss.last["pos"].cpu(), head._rel_loss.last["r_labels"].cpu().view(2, 8)
    assert torch.equal(pos[:n0], pos_clean[:n0].cpu()) and bool((pos[n0:] == -1).all())
    assert bool((lab[1] == 0).all()) and torch.equal(lab[0], torch.from_numpy(ref32["r_labels"]).view(2, 8)[0])
    assert torch.equal(head._rel_loss.last["row_loss"][:n0], row_clean[:n0])
    for k in ("subject_scores", "object_scores"):
        assert torch.equal(grads[k][0], g_clean[k][0]) and float(grads[k][1].abs().max()) == 0.0
    for k in clean:                                                # the segmentation terms: untouched
        if k not in BR.NAMES:
            assert torch.equal(out[k], clean[k]), k
    for k in ("cls", "mask_rows", "mask"):
        assert torch.equal(grads[k], g_clean[k])
    assert math.isfinite(float(out["loss_subject_match"])) and math.isfinite(float(out["loss_object_match"]))


def test_a_failed_last_layer_segmentation_assignment_propagates():
    from pairnet_amd import hip
    case, _ = BR.golden_case("a")
    head = _head(case)
    clean, g_clean = _full(head, case)
    pos_clean = head._rel_loss.last["pos"].clone()
    cls = case["cls"].clone()
    cls[1, 1, 0, 0] = float("nan")          # last layer, image 1: its class cost row is NaN
    out, grads = _full(head, case, cls=cls)
    assert int(head.seg_status().cpu()) != 0
    st = int(head.rel_status().cpu())
    assert st & hip.REL_STATUS_SEG and not st & ~hip.REL_STATUS_SEG
    n0 = min(8, case["gt_rels"][0].shape[0])
    pos, lab = head._rel_loss.last["pos"].cpu(), head._rel_loss.last["r_labels"].cpu().view(2, 8)
    assert torch.equal(pos[:n0], pos_clean[:n0].cpu()) and bool((pos[n0:] == -1).all())
    assert bool((lab[1] == 0).all()) and bool((lab[0] != 0).any())
    for k in ("subject_scores", "object_scores"):
        assert torch.equal(grads[k][0], g_clean[k][0]) and float(grads[k][1].abs().max()) == 0.0
    assert math.isfinite(float(out["loss_subject_match"])) and math.isfinite(float(out["r_loss_cls"]))


# ------------------------------------------------------------------------------ refusals
def test_images_without_relations_and_with_more_objects_than_queries_are_refused():
    case, _ = BR.golden_case("a")
    head = _head(case)
    with pytest.raises(ValueError, match="no ground-truth relation"):
        _full(head, case, gt_rels=[case["gt_rels"][0], torch.zeros(0, 3, dtype=torch.int64)])
    big = S.loss_case(2, 2, 8, 5, 13, 21, 50, (9, 2), 7)
    with pytest.raises(ValueError, match="queries"):
        _full(head, case, gt_labels=big["gt_labels"], gt_masks=big["gt_masks"],
              gt_rels=[torch.tensor([[0, 8, 1]]), case["gt_rels"][1]])
    assert head._seg_loss is None or head._seg_loss.last is None       # nothing was launched


# ------------------------------------------------------------------------------ interface
def test_detector_val_full_losses_equals_the_parts_run_by_hand():
    from helpers import baseline_cfg, head_cfg
    from pairnet_amd import BaselineRelationLoss, CrossHead2, CrossHeadBaseline, PSGTr
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
    gt_rels = [torch.tensor([[0, 1, 5], [2, 0, 17], [1, 2, 56]]), torch.tensor([[0, 1, 2], [1, 0, 30]])]
    g1 = {}
    got = det.val_full_losses(img, metas, gt_rels, gt_labels, raw, seed=4, step=2, grads=g1)
    got = {k: v.clone() for k, v in got.items()}
    assert len(got) == 30 and head.return_all_layers is False
    assert int(head.seg_status().cpu()) == 0 and int(head.rel_status().cpu()) == 0
    head.return_all_layers = True
    try:
        cls, masks = head.forward(det.extract_feat(img), metas)
    finally:
        head.return_all_layers = False
    g2 = {}
    want = head.seg_losses(cls, masks, gt_labels, det._prepare_gt_masks(img, raw), metas, seed=4, step=2,
                           grads=g2)
    rel = BaselineRelationLoss(head.num_relations, head.num_obj_query, head.num_rel_query)
    want.update(rel.loss(cls["rel"], cls["subject_scores"], cls["object_scores"], gt_rels,
                         head._seg_loss.last["matched"], 2, grads=g2, num_gts=[3, 2]))
    assert set(got) == set(want) and set(BR.NAMES) <= set(got)
    for k in want:
        assert torch.equal(got[k], want[k]) and math.isfinite(float(got[k])), k
    assert set(g1) == set(g2) and all(torch.equal(g1[k], g2[k]) for k in g2)
    assert tuple(g1["rel"].shape) == (2, 100, 57) and tuple(g1["subject_scores"].shape) == (2, 100, 100)
    with pytest.raises(NotImplementedError):                     # the other paths stay refused
        det.val_losses(img, metas, gt_rels, None, gt_labels, raw)
    det2 = PSGTr.from_parts(ResNet50Hip(depth=50), CrossHead2(**head_cfg()))
    with pytest.raises(NotImplementedError):                     # (refused before anything runs)
        det2.val_full_losses(img, metas, gt_rels, gt_labels, raw)
