"""Host: the float64 / integer statements of tests/post_ref.py pinned to torch and to the oracle
(oracle/head.py::_get_bboxes_single for the panoptic loop, oracle/deformable_detr.py and
oracle/bbox_head.py for the box trunk, the SinePositionalEncoding restatement of oracle/layers.py
for the padded sine encoding), and what tests/test_post_kernels_gpu.py relies on proved from the
reference alone: every "decisive" input of tests/post_cases.py is decisive (values on the 1/8
grid, the intended tie or edge present, the intended answer the reference's), and on the random
inputs at most 1 % of the rows / pixels have a float64 margin inside the value bound."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fwd_ref
import post_cases as K
import post_ref as R

U = R.U


def _close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), \
        float((a - b).abs().max())


def _on_grid(x):
    f = x[torch.isfinite(x)]
    return bool((f * 8 == (f * 8).round()).all())


# ============================================================ softmax family
@pytest.mark.parametrize("C,rows,seed", K.soft_cases())
def test_label_inputs_are_decisive_and_follow_torch(C, rows, seed):
    x = K.soft_input(C, rows, seed)
    assert _on_grid(x) and not R.soft_nan_rows(x).any()
    p64 = F.softmax(x.double(), -1)
    for off in (0, 1):
        label, score, mag, cond, bad = R.cls_argmax(x, off)
        want_s, want_i = p64[:, :C - 1].max(-1)
        assert torch.equal(label, want_i + off) and not bad.any()
        _close(score, want_s)
        assert bool(((label >= off) & (label <= off + C - 2)).all())
    # decisive: among the admitted logits the runner-up is either an exact tie (then the winner
    # is the first of them) or at least 1/8 below, i.e. its probability is lower by > 11 %
    adm = x[:, :C - 1].double()
    top = adm.amax(-1, keepdim=True)
    first = (adm == top).double().argmax(-1)
    assert torch.equal(first, R.cls_argmax(x, 0)[0])
    rest = torch.where(adm == top, torch.full_like(adm, -math.inf), adm)
    assert bool((top[:, 0] - rest.amax(-1) >= 0.125).all())


@pytest.mark.parametrize("C", [1] + K.SOFT_C)
def test_softmax_statements_match_torch(C):
    x = K.soft_input(C, 9, C, admitted=C)
    p, mag, cond = R.softmax(x)
    _close(p, F.softmax(x.double(), -1))
    assert bool((cond >= 0).all()) and bool(torch.isfinite(cond).all())
    out, omag, _ = R.rel_dists(x)
    _close(out, torch.cat([torch.zeros(9, 1, dtype=torch.float64), F.softmax(x.double(), -1)], -1))
    assert bool((out[:, 0] == 0).all()) and not bool(torch.signbit(out[:, 0]).any())


def test_crafted_rows_hold_what_they_claim():
    for C in K.SOFT_C:
        g = K.gen(C)
        A = C - 1
        x = K.soft_row(C, "excluded_max", g)
        assert int(x.argmax()) == C - 1 and int(x[:A].argmax()) != C - 1
        x = K.soft_row(C, "tie_ends", g)
        assert x[0] == x[A - 1] == x[:A].max()
        x = K.soft_row(C, "tie_lanes", g)
        w = torch.nonzero(x[:A] == x[:A].max())[:, 0]
        if A > 2:
            assert len(w) == 2 and (int(w[1]) - int(w[0])) % 64 != 0
        x = K.soft_row(C, "tie_lane", g)
        w = torch.nonzero(x[:A] == x[:A].max())[:, 0]
        if A > 64 + (A // 5) % 64:
            assert len(w) >= 2 and int(w[1]) - int(w[0]) == 64
        x = K.soft_row(C, "neg_inf", g)
        assert bool((x == -math.inf).any()) or C < 4
        x = K.soft_row(C, "spread100", g)
        assert float(x.max() - x.min()) >= 100.0 or C < 3
        assert math.exp(-100.0) < 2.0 ** -126          # the tail is below FLT_MIN


@pytest.mark.parametrize("C", [2, 3, 65, 134, 256])
def test_hostile_rows_rule(C):
    """Rows without a softmax: the label is torch.argmax of the admitted LOGITS where one of
    them is NaN (torch treats NaN as the maximum: the first one) and 0 otherwise; the score is
    NaN.  (torch's softmax of such a row is NaN throughout, whose argmax is 0.)"""
    x, want = K.hostile_rows(C)
    assert bool(R.soft_nan_rows(x).all())
    assert bool(torch.isnan(F.softmax(x, -1)).all())
    for off in (0, 1):
        label, score, _, _, bad = R.cls_argmax(x, off)
        assert bool(bad.all()) and bool(torch.isnan(score).all())
        assert torch.equal(label, want + off)
        assert bool(((label >= off) & (label <= off + C - 2)).all())
    nan_adm = torch.isnan(x[:, :C - 1]).any(-1)
    assert torch.equal(x[:, :C - 1].argmax(-1)[nan_adm], want[nan_adm])
    assert bool((want[~nan_adm] == 0).all())


def _o32_softmax(x):
    return F.softmax(x, -1)


@pytest.mark.parametrize("C,rows,seed", K.SOFT_RANDOM)
def test_random_label_rows_cap(C, rows, seed):
    """At most 1 % of the random rows have a runner-up within the value bound of the winner."""
    x = K.soft_random(C, rows, seed)
    p, mag, cond = R.softmax(x)
    bound, a = R.value_bound(p, mag, R.SOFT_L, cond, _o32_softmax(x))
    adm, badm = p[:, :C - 1], bound[:, :C - 1]
    top, i = adm.max(-1)
    rest = adm.clone()
    rest.scatter_(1, i[:, None], -1.0)
    close = (top[:, None] - rest) <= (badm + badm.gather(1, i[:, None]))
    close.scatter_(1, i[:, None], False)
    frac = float(close.any(-1).double().mean())
    print("C %d: a %.2f, rows with a runner-up inside the bound: %.4f" % (C, a, frac))
    assert frac <= 0.01


# ============================================================ row argmax, top-k
@pytest.mark.parametrize("n", K.ARGMAX_N)
def test_row_argmax_statement(n):
    for rows in K.ARGMAX_ROWS:
        x = K.argmax_input(n, rows, n)
        assert _on_grid(x)
        want = R.argmax_first(x.numpy())
        assert torch.equal(want, x.double().argmax(-1))         # torch: first index, -inf rows: 0
        assert bool((want[(x == -math.inf).all(-1)] == 0).all())


@pytest.mark.parametrize("n", [1, 2, 1023, 1025, 10241])
def test_topk_statement(n):
    for k in K.topk_ks(n, strided=True):
        for seed in range(0, 9, 3):
            x = K.topk_input(n, k, 3, seed)
            idx = R.topk(x.numpy(), k)
            vals, order = torch.sort(x.double() + 0.0, dim=-1, descending=True, stable=True)
            assert torch.equal(idx, order[:, :k])
            tv = torch.topk(x, k, dim=-1)[0]
            assert torch.equal(x.gather(1, idx) + 0.0, tv + 0.0)
            if k < n:       # nothing left out beats anything taken; ties go to the smaller index
                got = x.double().gather(1, idx)
                assert bool((got[:, 1:] <= got[:, :-1]).all())
                tie = got[:, 1:] == got[:, :-1]
                assert bool((idx[:, 1:] > idx[:, :-1])[tie].all())


def test_topk_rows_hold_what_they_claim():
    g = K.gen(1)
    n, k = 1025, 256
    x = K.topk_row(n, k, "two_valued", g)
    assert k < int((x == 0.75).sum()) < n
    x = K.topk_row(n, k, "signed_zero", g)
    assert bool(torch.signbit(x[x == 0]).any()) and bool((~torch.signbit(x[x == 0])).any())
    x = K.topk_row(n, k, "denormal", g)
    assert 0 < float(x.abs().max()) < 2.0 ** -126
    x = K.topk_row(n, k, "last_bit", g)
    assert float((x.unique()[1:] - x.unique()[:-1]).min()) == 2.0 ** -23
    x = K.topk_row(n, k, "kth_equal", g)
    s = torch.sort(x, descending=True)[0]
    assert s[k - 1] == s[k]
    for q in K.TOPK_Q:
        assert q * q <= 65536
    assert any(q * q <= 10240 for q in K.TOPK_Q) and any(10240 < q * q <= 24576 for q in K.TOPK_Q)
    assert any(24576 < q * q <= 40960 for q in K.TOPK_Q) and any(q * q > 40960 for q in K.TOPK_Q)


# ============================================================ panoptic
@pytest.mark.parametrize("n", K.PAN_N)
def test_panoptic_statement(n):
    for HW in K.PAN_HW:
        masks, labels, remap = K.panoptic_input(n, HW, 0)
        assert bool((masks == masks.round()).all())
        m_id = masks.double().argmax(0)
        seg, area = R.panoptic(masks, labels)
        assert torch.equal(seg, m_id * 1000 + labels[m_id])
        assert int(area.sum()) == HW
        seg2, area2 = R.panoptic(masks, labels, remap)
        r = remap.long()[m_id]
        assert torch.equal(seg2, r * 1000 + labels[r]) and int(area2.sum()) == HW
        if n > 1 and HW > 1:
            top = masks.amax(0)
            assert bool(((masks == top).sum(0) > 1).any())        # exact ties are present


def _oracle_pan(scene, all_cls):
    from oracle.head import OracleCrossHead2
    NC = scene["NC"]
    me = types.SimpleNamespace(num_classes=NC, num_relations=2, num_rel_query=1)
    h, w = scene["h"], scene["w"]
    z = torch.zeros
    out = OracleCrossHead2._get_bboxes_single(
        me, scene["masks"], all_cls, z(1, 3), z(1, 3), z(1, 2), z(1, h, w), z(1, h, w),
        (h, w, 3), [1.0, 1.0, 1.0, 1.0])
    return out[4]


def _scene_logits(scene):
    """Class logits whose torch softmax / max reproduces the scene's labels; the scores are
    what torch makes of them (0.5 exactly for two equal logits)."""
    Q, NC = scene["Q"], scene["NC"]
    lg = torch.full((Q, NC + 2), -math.inf)
    s = scene["scores"].double().clamp(1e-3, 1 - 1e-3)
    lg[torch.arange(Q), scene["labels"]] = (s / (1 - s)).log().float()
    lg[:, NC + 1] = 0.0
    return lg


@pytest.mark.parametrize("name", ["threshold", "merge", "nkeep0", "single", "ties"])
def test_panoptic_loop_matches_the_oracle(name):
    scene = K.pan_scenes()[name]
    lg = _scene_logits(scene)
    scores, ids = F.softmax(lg, -1)[..., :-1].max(-1)
    assert torch.equal(ids, scene["labels"])
    Q, h, w, NC = scene["Q"], scene["h"], scene["w"], scene["NC"]
    ref = R.panoptic_loop(scene["masks"].view(Q, -1).double().numpy(), ids, scores, NC - 1, 8)
    want = _oracle_pan(scene, lg)
    assert ref["active"] == 0 and ref["all_gone"] == 0
    assert np.array_equal(ref["seg"].reshape(h, w), want.numpy())


def test_panoptic_scenes_hold_what_they_claim():
    S = K.pan_scenes()

    def run(name, rounds=8):
        s = S[name]
        assert bool((s["masks"] == s["masks"].round()).all())
        return R.panoptic_loop(s["masks"].view(s["Q"], -1).double().numpy(), s["labels"],
                               s["scores"], s["NC"] - 1, rounds)
    t = run("threshold")
    s = S["threshold"]
    assert float(s["scores"][0]) == 0.5 and 0.5 < float(s["scores"][1]) < 0.5 + 1e-7
    assert t["kept"].tolist() == [1, 4] and int(s["labels"][3]) == s["NC"] - 1
    assert float(s["scores"][3]) > 0.5 and t["rounds"] == 0
    m = run("merge")
    assert m["klab"].tolist() == [79, 79, 80, 7, 80, 100]
    assert m["remap"].tolist() == [0, 1, 2, 3, 2, 5]          # 79 stays apart, 80 merges
    assert m["rounds"] == 2 and m["alive"].tolist() == [0, 1, 0, 1, 0, 1] and m["active"] == 0
    r1 = run("merge", 1)
    assert r1["rounds"] == 1 and r1["alive"].tolist() == [0, 1, 1, 1, 0, 1] and r1["active"] == 1
    seg1 = r1["seg"]
    assert int((seg1 == 0 * 1000 + 79).sum()) == 4 and int((seg1 == 1 * 1000 + 79).sum()) == 5
    assert int((seg1 == 2 * 1000 + 80).sum()) == 6           # 3 + 3 merged: survives round 1 only
    assert run("merge", 3)["active"] == 0 and run("merge", 2)["active"] == 1
    z = run("nkeep0")
    assert z["nkeep"] == 0 and bool((z["seg"] == 1).all()) and z["active"] == 0
    g = run("all_gone")
    assert g["nkeep"] == 3 and g["all_gone"] == 1 and g["active"] == 0 and not g["alive"].any()
    assert g["kept"].tolist() == [1, 100, 255]
    one = run("single")
    assert one["nkeep"] == 1 and one["rounds"] == 0
    ti = run("ties")
    assert ti["rounds"] == 2 and ti["alive"].tolist() == [1, 0, 0]


def _up_bound(scene):
    Q, ho, wo = scene["Q"], scene["ho"], scene["wo"]
    up, mag, spread = fwd_ref.bilinear(scene["masks"], ho, wo)
    o32 = F.interpolate(scene["masks"][None], (ho, wo), mode="bilinear", align_corners=False)[0]
    import fwd_cases
    extra = fwd_cases.bilinear_extra(scene["h"], scene["w"], spread)
    bound, a = R.value_bound(up, mag, fwd_cases.BIL_L, None, o32)
    return up.reshape(Q, -1), (bound + U * extra).reshape(Q, -1)


def test_upsampled_scene_cap():
    """The 7 x 9 -> 13 x 20 scene converges in its first round, and at most 1 % of its pixels
    have a second kept plane within the resize's value bound of the winner."""
    scene = K.pan_up_scene()
    up, bound = _up_bound(scene)
    ref = R.panoptic_loop(up.numpy(), scene["labels"], scene["scores"], scene["NC"] - 1, 4,
                          want_ids=True)
    assert ref["rounds"] == 0 and ref["active"] == 0 and ref["nkeep"] >= 3
    kept = torch.from_numpy(ref["kept"]).long()
    v, b = up[kept], bound[kept]
    top, i = v.max(0)
    close = (top[None] - v) <= (b + b.gather(0, i[None]))
    close.scatter_(0, i[None], False)
    assert float(close.any(0).double().mean()) <= 0.01


# ============================================================ box trunk glue
def test_zero_rows_needs_a_select():
    x, valid = K.zero_rows_input(2, 50, 4, 12, 0, True)
    ref = R.zero_rows(x, valid.expand(2, 50))
    assert not torch.isnan(ref).any() and not torch.signbit(ref[~valid.expand(2, 50)]).any()
    assert torch.isnan(x * valid.expand(2, 50)[..., None]).any()      # a product would not do


@pytest.mark.parametrize("rows", [1, 3, 300])
def test_box_pos_embed_statement(rows):
    from oracle.deformable_detr import DeformableDetrTransformer as T
    x = K.box_logits(rows, 0)
    s, emb, mag, cond = R.box_pos_embed(x)
    _close(s, x.double().sigmoid())
    want = T.get_proposal_pos_embed(x.double()[None])[0]
    assert float((emb - want).abs().max()) < 5e-6          # (the oracle's dim_t is fp32)
    o32 = T.get_proposal_pos_embed(x[None])[0]
    assert float((emb - o32.double()).abs().max()) < 1e-5
    assert float(cond.max()) <= R.POS_ARG_L * 2 * math.pi + 1e-9


@pytest.mark.parametrize("rows", [1, 64, 65])
def test_box_refine_statement(rows):
    from oracle.deformable_detr import inverse_sigmoid
    delta, ref_in = K.refine_input(rows, rows)
    out, mag, cond = R.box_refine(delta, ref_in)
    want = (delta.double() + inverse_sigmoid(ref_in.double())).sigmoid()
    _close(out, want)
    assert bool(torch.isfinite(cond).all()) and bool(torch.isfinite(out).all())
    if rows * 4 >= 40:
        pairs = set(zip(ref_in.view(-1).tolist(), delta.view(-1).tolist()))
        for r in K.REFINE_REF:
            for d in K.REFINE_DELTA:
                assert (float(torch.tensor(r)), d) in pairs


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_box_sampling_statement(L):
    B, rpi = 3, 5
    offaw, ref, vr = K.box_sampling_input(B, rpi, L, 4, 0)
    rows, NP = B * rpi, L * 4
    off = offaw[:, :8 * NP * 2].double().view(rows, 8, L, 4, 2)
    lg = offaw[:, 8 * NP * 2:8 * NP * 3].double().view(rows, 8, NP)
    for ratios in (None, vr):
        loc, lmag, aw, amag, acond = R.box_sampling(offaw, ref, L, ratios, rpi)
        _close(aw, F.softmax(lg, -1))
        r4 = ref.double()[:, None, :]                                        # [rows][1][4]
        if ratios is not None:      # reference_points[:, :, None] * cat([vr, vr], -1)[:, None]
            v = ratios.double().repeat_interleave(rpi, 0)
            r4 = ref.double()[:, None, :] * torch.cat([v, v], -1)
        else:
            r4 = r4.expand(rows, L, 4)
        want = r4[:, None, :, None, :2] + off / 4 * r4[:, None, :, None, 2:] * 0.5
        _close(loc, want.reshape(rows, 8, NP, 2))
        assert bool((lmag >= loc.abs() - 1e-12).all())
    assert len({float(v) for v in vr.view(-1)}) == B * L * 2                 # all distinct


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_token_sampling_statement(L):
    from oracle.deformable_detr import DeformableDetrTransformer as T
    offaw, vr, shapes = K.token_sampling_input(L, 2, 4, 0)
    loc, lmag, aw, amag, acond = R.token_sampling(offaw, vr, shapes)
    refp = T.get_reference_points(shapes, vr.double())                       # [B][N][L][2]
    NP = L * 4
    off = offaw[..., :8 * NP * 2].double().view(2, -1, 8, L, 4, 2)
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
    want = refp[:, :, None, :, None, :] + off / wh[None, None, None, :, None, :]
    _close(loc, want.reshape(2, -1, 8, NP, 2))
    edges = K.level_edges(shapes)
    assert edges[0] == 0 and edges[-1] == loc.shape[1] - 1 and len(edges) == 2 * L
    assert not torch.equal(vr[0], vr[1])


def test_query_score_statement():
    for B in K.QS_B:
        for Nq in K.QS_NQ:
            for C in (1, 65, 256):
                x = K.query_score_input(B, Nq, C, 0)
                s, mag, cond = R.query_score(x)
                _close(s, F.softmax(x.double(), dim=1).max(-1)[0])


@pytest.mark.parametrize("R_,C", [(1, 2), (3, 65), (100, 134), (2, 64)])
def test_box_triplets_statement(R_, C):
    from oracle.bbox_head import OracleCrossHeadBBox as H
    s_cls, o_cls, s_box, o_box = K.box_triplets_input(R_, C, 0)
    assert _on_grid(s_cls) and _on_grid(o_cls)
    me = types.SimpleNamespace(num_relations=2, num_rel_query=1)
    for rescale in (False, True):
        labels, det, mag, cond = R.box_triplets(s_cls, o_cls, s_box, o_box, 48.0, 80.0,
                                                K.TRIP_SF, rescale)
        out = H._get_bboxes_single(me, s_cls.double(), o_cls.double(), torch.zeros(1, 2),
                                   s_box.double(), o_box.double(), (48, 80, 3), K.TRIP_SF, rescale)
        _close(det, out[0])
        assert torch.equal(labels, out[1])
        assert bool((mag >= det.abs() - 1e-12).all())
    assert len(set(K.TRIP_SF)) == 4
    if R_ >= 3:     # boxes cross the image's edges, and one has no size
        x = torch.cat([s_box, o_box]).double()
        x1, x2 = (x[:, 0] - x[:, 2] / 2), (x[:, 0] + x[:, 2] / 2)
        y1, y2 = (x[:, 1] - x[:, 3] / 2), (x[:, 1] + x[:, 3] / 2)
        assert (x1 < 0).any() and (y1 < 0).any() and (x2 > 1).any() and (y2 > 1).any()
        assert ((x[:, 2] == 0) & (x[:, 3] == 0)).any()


@pytest.mark.parametrize("h,w", K.SINE_HW)
def test_sine_pe_statement(h, w):
    from oracle.layers import SinePositionalEncoding
    for C in K.SINE_C:
        for vh, vw in K.sine_valids(h, w):
            for offset in (0.0, -0.5):
                for T in (10000.0, 20.0):
                    out, mag, cond, wild = R.sine_pe(h, w, C, vh, vw, T, offset)
                    mask = torch.ones(1, h, w, dtype=torch.bool)
                    mask[:, :vh, :vw] = False
                    pe = SinePositionalEncoding(C // 2, temperature=T, normalize=True,
                                                offset=offset)(mask)
                    want = pe[0].permute(1, 2, 0).reshape(h * w, C).double()
                    ok = ~wild
                    assert float((out - want)[ok].abs().max()) < 2e-5 * (1 + float(cond[ok].max()))
                    assert bool(wild.any()) == (offset != 0 and (vh < h or vw < w))
                    assert float(cond[ok].max()) < 16.0 * (2 * math.pi + 1) * 2
    add = torch.randn(8, generator=K.gen(0))
    out, mag, _, _ = R.sine_pe(3, 5, 8, 3, 5, 20.0, 0.0, add)
    base, _, _, _ = R.sine_pe(3, 5, 8, 3, 5, 20.0, 0.0)
    _close(out, base + add.double())
