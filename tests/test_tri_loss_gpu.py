"""GPU: the triplet-matching kernels of csrc/tri_loss.hip alone, and the whole PSGTrHead2 loss
(pair-net_amd/psgtr2_losses.py), against the float64 statements of tests/tri_loss_ref.py and the
fixture tests/golden/tri_loss.npz (recorded from the reference's own loss).

Bound form (labnotes R14.2): |got - ref64| <= c * 2^-24 * mag + FLT_MIN per element, c = L_chain + a.
`mag` is the float64 computation on absolute values; `a`, the allowance for expf / logf / log1pf /
division, is twice the ratio the torch-fp32 run of the same statement reaches against its float64
run on the same inputs, and at least 4.  Nothing in c is measured from the kernel under test.

The cost cell (tri_loss_ref.cost_bound, K = ceil(Np / 256) + 10: a thread's fma chain over its
split's chunks, 6 butterfly steps, 3 wave additions and the splits' ordered sum, whatever the split
count) is bounded term by term -- mask K + 7, dice 2 K + 12,
class ceil(C / 64) + 14 + z -- each on its own term's magnitude, + 7 + a on the cell's magnitude for
the seven additions, + the first-order effect of the samples' own errors
(seg_loss_ref.sample_err through the analytic derivatives of tri_loss_ref.pair_prop).

The loss side reuses csrc/seg_loss.hip with one "layer" per side, so its bounds are those of
tests/test_seg_loss_gpu.py with L = 1 and Ml = M: loss_cls ceil(C / 64) + 2 rows + 14 +
ceil(ln C + 1); loss_mask K + 4 + M + 4; loss_dice 2 K + 10 + M + 4; the class gradients rows +
ceil(C / 64) + 14 + z; the mask gradients 4 K + 34 + n + 15 on mag, COORD roundings of the
coordinate scale beside it, and the samples' propagated error (tri_loss_ref.propagated)."""
import math

import numpy as np
import pytest
import torch

import seg_loss_ref as S
import tri_loss_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U, FLT_MIN = S.U, S.FLT_MIN
WORST = {}


def _hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip
    return hip


def _dev(t):
    return t.to(DEV).contiguous()


def _allow(v32, v64, mag):
    r = ((torch.as_tensor(v32).double() - torch.as_tensor(v64).double()).abs()
         / (U * torch.as_tensor(mag).double() + FLT_MIN))
    return max(4.0, 2.0 * float(r.max())) if r.numel() else 4.0


def _ratio(name, got, ref, mag, c):
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


# ------------------------------------------------------------------------------ the kernels alone
def _tables(case):
    """The device operands of the two entries for a case: (tab [B, 8], lsa_tab [B, 4], gt_rels,
    gt_labels, gt_masks, host offsets)."""
    B, Q = case["sub"].shape[1:3]
    R = [int(g.shape[0]) for g in case["gt_rels"]]
    G = [int(g.shape[0]) for g in case["gt_labels"]]
    tab, lsa, offs = [], [], []
    c = r = g = o = 0
    for b in range(B):
        tab += [c, R[b], r, g, G[b], o, 0, 0]
        lsa += [c, Q, R[b], o]
        offs.append((c, o))
        c, r, g, o = c + Q * R[b], r + R[b], g + G[b], o + min(Q, R[b])
    return (_dev(torch.tensor(tab).view(B, 8)), _dev(torch.tensor(lsa).view(B, 4)),
            _dev(torch.cat(case["gt_rels"]).long()), _dev(torch.cat(case["gt_labels"]).long()),
            _dev(torch.cat(case["gt_masks"])), dict(R=R, G=G, offs=offs, cells=c, M=o))


def _cost(case, pts=None):
    hip = _hip()
    B, Q = case["sub"].shape[1:3]
    tab, _, gr, gl, gm, hx = _tables(case)
    pts = torch.stack([p.reshape(-1, 2) for p in (pts or case["points"]["assign"])])
    cost = torch.full((hx["cells"],), float("nan"), device=DEV)
    scratch = hip.tri_match_cost(_dev(case["sub"][0]), _dev(case["obj"][0]), _dev(case["rel"][0]),
                                 _dev(case["sub_seg"][0]), _dev(case["obj_seg"][0]), gm, _dev(pts), gr,
                                 gl, tab, list(T.CFG["cost"]) + list(T.CFG["cost_eps"]), max(hx["G"]),
                                 Q * max(hx["R"]), cost)
    torch.cuda.synchronize()
    blocks = [cost[c:c + Q * r].view(Q, r).cpu() for (c, _), r in zip(hx["offs"], hx["R"])]
    return blocks, cost, scratch


def _check_cost(name, case, blocks, pts=None):
    for b, got in enumerate(blocks):
        p = None if pts is None else pts[b]
        r64, r32 = T.image_cost(case, b, pts=p), T.image_cost(case, b, torch.float32, pts=p)
        bound, a = T.cost_bound(case, b, r64, r32, pts=p)
        assert bool(torch.isfinite(got).all()), (name, b)
        err = (got.double() - r64["cost"]).abs()
        ratio = float((err / (U * r64["mag"] + FLT_MIN)).max())
        WORST["cost " + name] = max(WORST.get("cost " + name, 0.0), ratio)
        print("cost %s image %d: worst ratio %.3f against mag, %.4f of its bound (a = %.1f)"
              % (name, b, ratio, float((err / bound).max()), a))
        assert bool((err <= bound).all()), (name, b, ratio)


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_match_cost_alone_against_the_float64_statement(name):
    case = T.tri_case(**T.CASES[name])
    blocks, flat, scratch = _cost(case)
    _check_cost(name, case, blocks)
    again, flat2, _ = _cost(case)
    assert torch.equal(flat, flat2)                              # bitwise on two calls
    # the ground-truth samples are the existing sampler's, bit for bit
    hip = _hip()
    for b, gm in enumerate(case["gt_masks"]):
        want = torch.empty(gm.shape[0], case["num_points"], device=DEV)
        hip.point_sample(_dev(gm), _dev(case["points"]["assign"][b]), want)
        g0 = sum(m.shape[0] for m in case["gt_masks"][:b])
        assert torch.equal(scratch["t"][g0:g0 + gm.shape[0]], want)


def test_targets_exactly_and_the_device_side_range_check():
    hip = _hip()
    case = T.tri_case(**T.CASES["small"])
    B, Q, C, Cr = 2, 8, 5, 4
    tab, _, gr, gl, _, hx = _tables(case)
    M = hx["M"]
    rows = [np.array([q for q, _ in case["planted"][b]]) for b in range(B)]
    cols = [np.array([j for _, j in case["planted"][b]]) for b in range(B)]

    def run(gr_dev, lsa_status, gl_dev=gl):
        labels = torch.full((3, B * Q), -7, dtype=torch.int64, device=DEV)
        matched = torch.full((M, 4), -7, dtype=torch.int64, device=DEV)
        side = torch.full((2, M, 4), -7, dtype=torch.int64, device=DEV)
        rel_idx = torch.full((M,), -7, dtype=torch.int64, device=DEV)
        mcount, status = torch.full((1,), -7, dtype=torch.int32, device=DEV), \
            torch.full((1,), -7, dtype=torch.int32, device=DEV)
        hip.tri_targets(tab, _dev(torch.tensor(np.concatenate(rows), dtype=torch.int32)),
                        _dev(torch.tensor(np.concatenate(cols), dtype=torch.int32)),
                        _dev(torch.tensor(lsa_status, dtype=torch.int32)), gr_dev, gl_dev, Q, C, Cr,
                        labels, matched, side, rel_idx, mcount, status)
        torch.cuda.synchronize()
        return [t.cpu() for t in (labels, matched, side, rel_idx, mcount, status)]
    labels, matched, side, rel_idx, mcount, status = run(gr, [0, 0])
    want = T.targets(rows, cols, case["gt_rels"], case["gt_labels"], Q, C, Cr)
    assert torch.equal(labels, want[0]) and torch.equal(matched, want[1]) and torch.equal(rel_idx, want[2])
    assert int(mcount) == M and int(status) == 0
    for s in range(2):
        assert torch.equal(side[s][:, 0], torch.zeros(M, dtype=torch.int64))
        assert torch.equal(side[s][:, 1:3], matched[:, :2]) and torch.equal(side[s][:, 3], matched[:, 2 + s])
    # an image whose assignment failed keeps its fills and its rows -1; the other image is written
    labels, matched, side, rel_idx, mcount, status = run(gr, [1, 0])
    want = T.targets([None, rows[1]], [None, cols[1]], case["gt_rels"], case["gt_labels"], Q, C, Cr)
    assert torch.equal(labels, want[0]) and torch.equal(matched, want[1]) and torch.equal(rel_idx, want[2])
    assert int(mcount) == 3 and int(status) == 1 and bool((side[:, :5] == -1).all())
    # gt_rels on the device are range-checked there: object, predicate 0, predicate above Cr, label
    for (i, j, v) in ((5, 0, 3), (6, 2, 0), (7, 2, Cr + 1), (1, 1, -1)):
        bad = torch.cat(case["gt_rels"]).long()
        bad[i, j] = v
        labels, matched, _, _, mcount, status = run(_dev(bad), [0, 0])
        b = 0 if i < 5 else 1
        assert int(status) == hip.TRI_STATUS_RANGE
        lab = labels.view(3, B, Q)
        assert bool((lab[:2, b] == C).all()) and bool((lab[2, b] == Cr).all())
        assert torch.equal(lab[:, 1 - b], T.targets(rows, cols, case["gt_rels"], case["gt_labels"],
                                                    Q, C, Cr)[0].view(3, B, Q)[:, 1 - b])
        assert int(mcount) == (3 if b == 0 else 5) and bool((matched[:, 0] != b).all())
    bad_l = torch.cat(case["gt_labels"]).long()
    bad_l[0] = C
    assert int(run(gr, [0, 0], _dev(bad_l))[5]) == hip.TRI_STATUS_RANGE


# ------------------------------------------------------------------------------ the whole loss
def _loss_obj(case):
    from pairnet_amd import PSGTrHead2Loss
    return PSGTrHead2Loss(case["num_classes"], case["num_relations"], case["sub"].shape[2],
                          train_cfg=T.train_cfg(case["num_points"]))


def _run(case, points=None, obj=None, debug=True, **kw):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    obj = obj or _loss_obj(case)
    grads = {}
    B = case["sub"].shape[1]
    out = obj.loss({k: _dev(case[k]) for k in ("sub", "obj", "rel")},
                   {k: _dev(case[k]) for k in ("sub_seg", "obj_seg")}, case["gt_rels"], None,
                   case["gt_labels"], case["gt_masks"], [dict()] * B, grads=grads,
                   points=case["points"] if points is None else points, debug=debug, **kw)
    torch.cuda.synchronize()
    return obj, out, grads


def _check_whole(name, case, obj, out, grads, r, r32, ref32=None, gradients=True):
    B, Q = case["sub"].shape[1:3]
    h, w = case["sub_seg"].shape[-2:]
    C1, Cr1 = case["num_classes"] + 1, case["num_relations"] + 1
    M = r["matched"].shape[0]
    assert int(obj.assign_status.cpu()) == 0 and obj.last_on_device
    assert torch.equal(obj.last["matched"].cpu(), r["matched"])        # the planted assignments
    assert torch.equal(obj.last["rel_idx"].cpu(), r["rel_idx"])
    for i, k in enumerate(("sub_labels", "obj_labels", "rel_labels")):
        assert torch.equal(obj.last[k].cpu(), r["labels"][i]), k
    assert torch.equal(grads["mask_rows"].cpu(), r["mask_rows"]) and int(obj.last["mcount"].cpu()) == M
    assert obj.last["counts"] == [min(Q, g.shape[0]) for g in case["gt_rels"]]
    assert set(out) == set(T.NAMES) and all(v.dim() == 0 and v.is_cuda for v in out.values())
    Np = r["sides"][0]["pts"].shape[1]
    K = math.ceil(Np / 256) + 10
    ce = lambda c: math.ceil(c / 64) + 2 * B * Q + 14 + math.ceil(math.log(c) + 1)
    chain = dict(s_loss_cls=ce(C1), o_loss_cls=ce(C1), r_loss_cls=ce(Cr1))
    prop, g_prop = {}, []
    for s, n in enumerate("so"):
        chain[n + "_loss_mask"], chain[n + "_loss_dice"] = K + 4 + M + 4, 2 * K + 10 + M + 4
        pm, pd, gp = T.propagated(case, r, s, coefficients=gradients)
        prop[n + "_loss_mask"], prop[n + "_loss_dice"] = pm, pd
        g_prop.append(gp)
    for k in T.NAMES:
        ref, mag = float(r["losses"][k]), float(r["mags"][k])
        a = _allow(r32["losses"][k], ref, mag)
        err = abs(float(out[k]) - ref)
        bound = (chain[k] + a) * U * mag + prop.get(k, 0.0) + FLT_MIN
        WORST["%s %s" % (name, k)] = err / (U * mag + FLT_MIN)
        print("%s %s: ratio %.3f, bound %.3f roundings" % (name, k, err / (U * mag + FLT_MIN),
                                                           bound / (U * mag + FLT_MIN)))
        assert math.isfinite(float(out[k])) and err <= bound, (name, k, err, bound)
        if ref32 is not None:      # against the reference's own fp32 value: c plus its stored ratio
            i = list(ref32["names"]).index(k)
            assert abs(float(out[k]) - float(ref32["loss32"][i])) <= \
                bound + float(ref32["loss_ratio"][i]) * U * mag, (name, k)
    if not gradients:
        return
    for key, c in (("sub", C1), ("obj", C1), ("rel", Cr1)):
        x64 = case[key].double()
        z = (x64.amax(-1, keepdim=True) - x64).clamp(max=88.0)
        g64, gmag = r["g_" + key], r["g_%s_mag" % key]
        assert tuple(grads[key].shape) == tuple(case[key].shape)
        _ratio("%s g_%s" % (name, key), grads[key], g64, gmag,
               B * Q + math.ceil(c / 64) + 14 + z + _allow(r32["g_" + key], g64, gmag))
        if ref32 is not None:
            err = (grads[key].cpu().double() - torch.from_numpy(ref32["g_%s32" % key]).double()).abs()
            cc = B * Q + math.ceil(c / 64) + 14 + z + 4 + 2 * float(ref32["g_%s_ratio" % key])
            assert bool((err <= cc * U * gmag + FLT_MIN).all()), key
    for s, key in enumerate(("sub", "obj")):
        sd, sd32 = r["sides"][s], r32["sides"][s]
        got = grads[key + "_mask"]
        assert tuple(got.shape) == (M, h, w)
        cnt = S.scatter(torch.ones(M, Np), sd["pts"], h, w)[2]
        scale = sd["g_mask_mag"] + S.COORD * sd["g_mask_coord"]
        a = _allow(sd32["g_mask"], sd["g_mask"], scale)
        err = (got.cpu().double() - sd["g_mask"]).abs()
        bound = (4 * K + 34 + cnt + 15 + a) * U * sd["g_mask_mag"] + S.COORD * U * sd["g_mask_coord"] \
            + g_prop[s] + FLT_MIN
        ratio = float((err / (U * sd["g_mask_mag"] + FLT_MIN)).max())
        WORST["%s g_%s_mask" % (name, key)] = ratio
        print("%s g_%s_mask: worst ratio %.3f against mag alone, %.4f of its bound"
              % (name, key, ratio, float((err / bound).max())))
        assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), (name, key, ratio)
        if ref32 is not None:
            err = (got.cpu().double() - torch.from_numpy(ref32["g_%s_mask32" % key]).double()).abs()
            assert bool((err <= bound + float(ref32["g_%s_mask_ratio" % key]) * U * scale).all()), key


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("form", ["candidates", "loss"])
def test_whole_loss_on_the_fixture(name, form):
    case, ref32 = T.golden_case(name)
    pts = case["points"]
    if form == "loss":
        r0 = T.whole_loss(case, grad=False)            # (the float64 statement's final loss points)
        pts = dict(assign=pts["assign"], sub_loss=r0["sides"][0]["pts"], obj_loss=r0["sides"][1]["pts"])
    obj, out, grads = _run(case, pts)
    r, r32 = T.whole_loss(case, pts), T.whole_loss(case, pts, torch.float32)
    assert np.array_equal(r["matched"].numpy(), ref32["matched"])
    assert np.array_equal(r["rel_idx"].numpy(), ref32["rel_idx"])
    if form == "candidates":
        for s, k in enumerate(("sub", "obj")):
            assert torch.equal(obj.last[k + "_points"].cpu(), r["sides"][s]["pts"])
    blocks = [obj.last["cost"][c:c + 8 * g.shape[0]].view(8, -1).cpu()
              for c, g in zip((0, 8 * case["gt_rels"][0].shape[0]), case["gt_rels"])]
    _check_cost("fixture " + name, case, blocks)
    _check_whole("fixture %s/%s" % (name, form), case, obj, out, grads, r, r32, ref32)


@pytest.mark.parametrize("name", ["r_gt_q", "wide"])
def test_whole_loss_on_drawn_cases(name):
    case = T.tri_case(**T.CASES[name])
    obj, out, grads = _run(case)
    r, r32 = T.whole_loss(case), T.whole_loss(case, dtype=torch.float32)
    for b, pairs in case["planted"].items():
        rows = r["matched"][r["matched"][:, 0] == b]
        assert [int(q) for q in rows[:, 1]] == [q for q, _ in pairs]
        assert r["rel_idx"][r["matched"][:, 0] == b].tolist() == [j for _, j in pairs]
    _check_whole(name, case, obj, out, grads, r, r32)


def test_nan_in_one_mask_logit_sets_the_status_and_leaves_the_other_image_alone():
    case = T.tri_case(**T.CASES["small"])
    obj, clean, g_clean = _run(case)
    keep = {k: v.cpu().clone() for k, v in obj.last.items() if k in ("sub_labels", "obj_labels", "rel_labels")}
    bad = dict(case, obj_seg=case["obj_seg"].clone())
    px, py = case["points"]["assign"][1][0].tolist()          # a pixel image 1's first assign point reads
    bad["obj_seg"][0, 1, 3, min(12, max(0, math.floor(py * 13 - 0.5) + 1)),
                   min(20, max(0, math.floor(px * 21 - 0.5) + 1))] = float("nan")
    obj2, out, grads = _run(bad)
    assert int(obj2.assign_status.cpu()) == 1                                # pn_lsa_f32: a NaN entry
    for k, fill in (("sub_labels", 5), ("obj_labels", 5), ("rel_labels", 4)):
        lab = obj2.last[k].cpu().view(2, 8)
        assert bool((lab[1] == fill).all()) and torch.equal(lab[0], keep[k].view(2, 8)[0]), k
    m = obj2.last["matched"].cpu()
    assert bool((m[5:] == -1).all()) and bool((m[:5, 0] == 0).all())
    assert bool((grads["mask_rows"].cpu()[5:] == -1).all()) and int(obj2.last["mcount"].cpu()) == 5
    for k in T.NAMES:
        assert math.isfinite(float(out[k])), k
    for k, g in grads.items():
        assert bool(torch.isfinite(g.double()).all()), k
    assert float(grads["sub_mask"][5:].abs().max()) == 0.0 and float(grads["obj_mask"][5:].abs().max()) == 0.0
    # image 0's rows are the clean run's rows, bit for bit (its own normaliser aside: the loss VALUES
    # see 5 matched masks where the clean run saw 8)
    assert torch.equal(grads["mask_rows"][:5], g_clean["mask_rows"][:5])
    assert torch.equal(obj2.last["sub_points"][:5], obj.last["sub_points"][:5])


def test_same_seed_and_step_give_the_same_bits_and_another_step_other_points():
    case = T.tri_case(**T.CASES["r_gt_q"])
    none = dict()
    obj, o1, g1 = _run(case, none, seed=5, step=3)
    p1 = {k: obj.last[k].clone() for k in ("assign", "sub_points", "obj_points", "sub_candidates")}
    _, o2, g2 = _run(case, none, obj=obj, seed=5, step=3)
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    assert all(torch.equal(p1[k], obj.last[k]) for k in p1)
    _run(case, none, obj=obj, seed=5, step=4)
    assert all(not torch.equal(p1[k], obj.last[k]) for k in p1)
    assert not torch.equal(p1["sub_points"], p1["obj_points"])
    # the drawn points are the host Philox's at the five sites
    hip = _hip()
    M, Sn = 5, 150
    want = S.uniform(M * Sn * 2, 5, 0, hip.TRI_SITE_OBJ_CANDIDATES, 4)
    assert np.array_equal(obj.last["obj_candidates"].cpu().numpy().reshape(-1), want)
    want = S.uniform(2 * 50 * 2, 5, 0, hip.TRI_SITE_ASSIGN, 4)
    assert np.array_equal(obj.last["assign"].cpu().numpy().reshape(-1), want)


def test_two_calls_give_bitwise_equal_results():
    case = T.tri_case(**T.CASES["wide"])
    obj, o1, g1 = _run(case)
    c1 = obj.last["cost"].clone()
    _, o2, g2 = _run(case, obj=obj)
    assert torch.equal(c1, obj.last["cost"])
    assert all(torch.equal(o1[k], o2[k]) for k in o1) and all(torch.equal(g1[k], g2[k]) for k in g1)


def test_production_shape_call():
    """B 2, Q 100, C 133, Cr 56, 200 x 334 logits, 400 x 668 masks, Np 12 544, (15, 14) objects and
    (30, 29) relations: finite values that stayed on the device, no host scipy, the cost blocks
    within their bound of the float64 statement, the planted assignment found."""
    case = T.tri_case(**T.PRODUCTION)
    obj, out, grads = _run(case, dict(), seed=1, step=1)
    assert int(obj.assign_status.cpu()) == 0 and obj.last_on_device
    assert all(v.is_cuda and v.dim() == 0 and math.isfinite(float(v)) for v in out.values())
    assert all(bool(torch.isfinite(g.double()).all()) for g in grads.values())
    pts = [p.cpu() for p in obj.last["assign"]]
    Q, R = 100, [int(g.shape[0]) for g in case["gt_rels"]]
    blocks = [obj.last["cost"][c:c + Q * r].view(Q, r).cpu() for c, r in zip((0, Q * R[0]), R)]
    _check_cost("production", case, blocks, pts)
    m = obj.last["matched"].cpu()
    for b, pairs in case["planted"].items():
        assert m[m[:, 0] == b][:, 1].tolist() == [q for q, _ in pairs]
        assert obj.last["rel_idx"].cpu()[m[:, 0] == b].tolist() == [j for _, j in pairs]
    assert tuple(grads["sub_mask"].shape) == (59, 200, 334) and grads["mask_rows"].numel() == 59


# ------------------------------------------------------------------------------ interface
def test_head_triplet_losses_equal_the_loss_object_bitwise():
    from helpers import psgtr2_cfg
    from oracle import seeded
    from pairnet_amd import PSGTrHead2, PSGTrHead2Loss
    H, W, bs = 96, 128, 2
    head = PSGTrHead2(**psgtr2_cfg())
    head.init_weights(seed=3)
    head.to(DEV)
    feats = seeded.seeded_feats(7, bs, H, W)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[2.0] * 4)] * bs
    cls, masks = head.forward([f.to(DEV) for f in feats], metas)
    _, B, Q, h, w = masks["sub_seg"].shape
    g = torch.Generator().manual_seed(3)
    gt_labels = [torch.randint(0, 133, (3,), generator=g) for _ in range(bs)]
    gt_masks = [(torch.rand(3, 2 * h, 2 * w, generator=g) > 0.5).to(torch.uint8) for _ in range(bs)]
    gt_rels = [torch.tensor([[0, 1, 5], [0, 1, 56], [2, 2, 1]]), torch.tensor([[1, 0, 30]])]
    g1, g2 = {}, {}
    got = head.triplet_losses(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, grads=g1, seed=2, step=9)
    want = PSGTrHead2Loss(133, 56, Q).loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas,
                                           grads=g2, seed=2, step=9)
    assert set(got) == set(T.NAMES) and (B, Q) == (bs, 100)
    for k in want:
        assert torch.equal(got[k], want[k]) and math.isfinite(float(got[k])), k
    assert set(g1) == {"sub", "obj", "rel", "mask_rows", "sub_mask", "obj_mask"}
    assert all(torch.equal(g1[k], g2[k]) for k in g2)
    assert int(head.triplet_status().cpu()) == 0 and tuple(g1["sub_mask"].shape) == (4, h, w)


def test_detector_val_triplet_losses_runs_and_val_losses_still_refuses():
    from helpers import psgtr2_cfg
    from pairnet_amd import HalfSizeMasks, PSGTr, PSGTrHead2
    from pairnet_amd.backbone import ResNet50Hip
    H, W = 96, 128
    head = PSGTrHead2(**psgtr2_cfg())
    head.init_weights(seed=3)
    det = PSGTr.from_parts(ResNet50Hip(depth=50), head).to(DEV)
    g = torch.Generator().manual_seed(11)
    img = torch.randn(2, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(90, 120, 3), scale_factor=[2.0] * 4, batch_input_shape=(H, W))] * 2
    gt_labels = [torch.tensor([3, 17, 90]), torch.tensor([5, 60])]
    raw = [(torch.rand(3, 90, 120, generator=g) > 0.6).numpy().astype(np.uint8),
           (torch.rand(2, 90, 120, generator=g) > 0.5).numpy().astype(np.uint8)]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 0, 17]]), torch.tensor([[1, 0, 56]])]
    a = det.val_triplet_losses(img, metas, gt_rels, gt_labels, raw, seed=4, step=2)
    half = [HalfSizeMasks(m, (H, W)) for m in det._prepare_gt_masks(img, raw)]
    b = det.val_triplet_losses(img, metas, gt_rels, gt_labels, half, seed=4, step=2)
    assert set(a) == set(T.NAMES) and int(head.triplet_status().cpu()) == 0
    for k in a:
        assert torch.equal(a[k], b[k]) and math.isfinite(float(a[k])), k
    with pytest.raises(ValueError, match="image 1 has no ground-truth relation"):
        det.val_triplet_losses(img, metas, [gt_rels[0], torch.zeros(0, 3, dtype=torch.int64)], gt_labels, raw)
    with pytest.raises(NotImplementedError):                     # the other entries keep their refusals
        det.val_losses(img, metas, gt_rels, None, gt_labels, raw)
    with pytest.raises(NotImplementedError):
        det.val_seg_losses(img, metas, gt_labels, raw)
    with pytest.raises(NotImplementedError):
        det.val_full_losses(img, metas, gt_rels, gt_labels, raw)
    with pytest.raises(NotImplementedError):
        det.trainer()
