"""float64 statement of the sibling head's relation losses (csrc/rel_loss.hip,
pair-net_amd/baseline_losses.py), written from the reference's steps (relation_heads/baseline.py:
655-694, 828-907 with OldIdMatcher, approaches/matcher.py:279-351, and MultilabelCrossEntropy,
losses/seg_losses.py:47-57) and sharing no code with the kernels' Python, plus the case builders
the CPU and GPU tests share and `run_reference`, which executes the reference's OWN
`CrossHeadBaseline.loss` in place (present on build machines only) the way
seg_loss_ref.run_reference executes `MaskFormerHead.loss`.  Every function takes `dtype`: float64 is
the reference, float32 the torch-fp32 oracle whose own error sets the allowance `a` of the bounds.
The segmentation matching the relation terms rest on is seg_loss_ref.whole_loss's."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

import seg_loss_ref as S

U, FLT_MIN, EPS32 = S.U, S.FLT_MIN, S.EPS32
REL_CFG = dict(c_sub=1.0, c_obj=1.0, c_rel=1.0, w_rel=2.0, w_sub=2.0, w_obj=2.0)
NAMES = ("r_loss_cls", "loss_subject_match", "loss_object_match")


# ------------------------------------------------------------------------------ pieces
def assigned_queries(G, od_pos, gt_inds):
    """Step 1: a = ones(G); a[pos_assigned_gt_inds] = od_pos_inds (the fill is 1, baseline.py:829)."""
    a = torch.ones(G, dtype=torch.int64)
    a[torch.as_tensor(gt_inds, dtype=torch.int64)] = torch.as_tensor(od_pos, dtype=torch.int64)
    return a


def id_cost(rel, sub, obj, gt_rels, a, cfg=REL_CFG, dtype=torch.float64):
    """Steps 2-3 for one image: rel [R][C1], sub / obj [R][Q], gt_rels [Gr][3], a [G] ->
    (cost [R][Gr], mag [R][Gr] = the sum of the three weighted softmax entries)."""
    gs, go, gr = a[gt_rels[:, 0]], a[gt_rels[:, 1]], gt_rels[:, 2]
    ps = torch.softmax(sub.to(dtype), -1)[:, gs] * cfg["c_sub"]
    po = torch.softmax(obj.to(dtype), -1)[:, go] * cfg["c_obj"]
    pr = torch.softmax(rel.to(dtype), -1)[:, gr] * cfg["c_rel"]
    return (-ps - po) - pr, ps + po + pr


def cost_z(rel, sub, obj, gt_rels, a):
    """max x - x[entry] of the three softmax entries each cost element reads, capped at 88: the
    roundings the subtraction in front of expf costs (R14.2's z), [R][Gr]."""
    out = None
    for x, idx in ((sub, a[gt_rels[:, 0]]), (obj, a[gt_rels[:, 1]]), (rel, gt_rels[:, 2])):
        x = x.double()
        z = (x.amax(-1, keepdim=True) - x[:, idx]).clamp(max=88.0)
        out = z if out is None else torch.maximum(out, z)
    return out


def id_ce(scores, rows, cols, tgt, w, B, dtype=torch.float64):
    """Step 6 for one image: -log_softmax(scores[rows][:, cols])[i, tgt_i], mean over i, times w,
    over B (the batch mean's share) -> (value, mag, the smallest row magnitude where there is more than one
    column); differentiable in scores."""
    f = scores.to(dtype)[rows][:, cols]
    lse = torch.logsumexp(f, -1)
    xt = f[torch.arange(len(rows)), tgt]
    P = len(rows)
    m = f.amax(-1)
    row_mag = m.abs() + (lse - m) + xt.abs()         # the summands of lse - x_t: m + log d - x_t
    lo = float(row_mag.detach().min()) if len(cols) > 1 else float("inf")   # (one column: exact)
    return w * ((lse - xt).sum() / P) / B, w * (row_mag.sum() / P) / B, lo


def relation_loss(rel, sub, obj, gt_rels, od, G, class_weight, cfg=REL_CFG, dtype=torch.float64,
                  grad=True, assignment=None):
    """Steps 1-7 over the batch.  rel [B][R][C1], sub / obj [B][R][Q] fp32, gt_rels[b] [Gr_b][3],
    od[b] = (od_pos_inds ascending, pos_assigned_gt_inds), G[b].  -> dict(losses, mags, g_rel, g_sub,
    g_obj and their *_mag, costs [b], cost_mags, pairs [b] = (rows, cols), r_labels [B*R], pos
    [P][4])."""
    B, R, C1 = rel.shape
    rel_v = rel.detach().to(dtype).requires_grad_(grad)
    sub_v = sub.detach().to(dtype).requires_grad_(grad)
    obj_v = obj.detach().to(dtype).requires_grad_(grad)
    r_labels = torch.zeros(B, R, dtype=torch.int64)
    costs, cmags, pairs, pos, zs = [], [], [], [], []
    l_sub = l_obj = m_sub = m_obj = 0.0
    row_mag_min = float("inf")
    g_sub_mag, g_obj_mag = torch.zeros_like(sub, dtype=dtype), torch.zeros_like(obj, dtype=dtype)
    for b in range(B):
        gr = torch.as_tensor(gt_rels[b]).long()
        od_pos = torch.as_tensor(od[b][0]).long()
        a = assigned_queries(G[b], od_pos, od[b][1])
        with torch.no_grad():
            cost, cmag = id_cost(rel[b], sub[b], obj[b], gr, a, cfg, dtype)
            if assignment is not None:
                rows, cols = assignment[b]
            else:
                rows, cols = linear_sum_assignment(cost.numpy())
            order = np.argsort(rows)
            rows, cols = np.asarray(rows)[order], np.asarray(cols)[order]
        costs.append(cost), cmags.append(cmag), pairs.append((rows, cols))
        zs.append(cost_z(rel[b], sub[b], obj[b], gr, a))
        r_labels[b, rows] = gr[cols, 2]
        where = {int(q): j for j, q in enumerate(od_pos.tolist())}
        ts = torch.tensor([where[int(a[gr[k, 0]])] for k in cols])      # KeyError: the reference raises
        to = torch.tensor([where[int(a[gr[k, 1]])] for k in cols])
        for i, r in enumerate(rows):
            pos.append((b, int(r), int(ts[i]), int(to[i])))
        v, m, lo = id_ce(sub_v[b], rows, od_pos, ts, cfg["w_sub"], B, dtype)
        l_sub, m_sub, row_mag_min = l_sub + v, m_sub + m.detach(), min(row_mag_min, lo)
        v, m, lo = id_ce(obj_v[b], rows, od_pos, to, cfg["w_obj"], B, dtype)
        l_obj, m_obj, row_mag_min = l_obj + v, m_obj + m.detach(), min(row_mag_min, lo)
        with torch.no_grad():      # |softmax| + |onehot| times the scale
            for sc, tg, w, dst in ((sub, ts, cfg["w_sub"], g_sub_mag), (obj, to, cfg["w_obj"], g_obj_mag)):
                f = torch.softmax(sc[b].to(dtype)[rows][:, od_pos], -1) + F.one_hot(tg, len(od_pos))
                blk = torch.zeros(len(rows), sc.shape[-1], dtype=dtype)
                blk[:, od_pos] = f * (w / (B * len(rows)))
                dst[b, rows] = blk
    l_rel, m_rel = S.ce_avg(rel_v.view(1, B * R, C1), r_labels.view(1, B * R), class_weight,
                            cfg["w_rel"], dtype)
    losses = dict(r_loss_cls=l_rel[0], loss_subject_match=l_sub, loss_object_match=l_obj)
    out = dict(losses={k: v.detach() for k, v in losses.items()},
               mags=dict(r_loss_cls=m_rel[0].detach(), loss_subject_match=m_sub, loss_object_match=m_obj),
               row_mag_min=row_mag_min, costs=costs, cost_mags=cmags, cost_z=zs, pairs=pairs, r_labels=r_labels.view(-1),
               pos=torch.tensor(pos, dtype=torch.int64).reshape(-1, 4))
    if grad:
        (l_rel[0] + l_sub + l_obj).backward()
        out.update(g_rel=rel_v.grad.detach(), g_sub=sub_v.grad.detach(), g_obj=obj_v.grad.detach(),
                   g_rel_mag=S.ce_avg_grad(rel.view(1, B * R, C1), r_labels.view(1, B * R),
                                           class_weight, cfg["w_rel"], dtype)[1].view(B, R, C1),
                   g_sub_mag=g_sub_mag, g_obj_mag=g_obj_mag)
    return out


def od_of(matched, L, B, gt_labels):
    """The last layer's (od_pos_inds, pos_assigned_gt_inds) per image from whole_loss's matched rows."""
    G = [int(g.shape[0]) for g in gt_labels]
    goff = np.concatenate([[0], np.cumsum(G)])
    od = []
    for b in range(B):
        rows = matched[(matched[:, 0] == L - 1) & (matched[:, 1] == b)]
        od.append((rows[:, 2].clone(), rows[:, 3] - int(goff[b])))
    return od, G


def run_whole(case, dtype=torch.float64, grad=True):
    """The full 30-key statement: seg_loss_ref.whole_loss, then the relation terms on its last
    layer's matching -> (the segmentation dict, the relation dict)."""
    seg = S.run_whole(case, dtype=dtype, grad=grad)
    L, B = case["cls"].shape[:2]
    od, G = od_of(seg["matched"], L, B, case["gt_labels"])
    r = relation_loss(case["rel"], case["sub"], case["obj"], case["gt_rels"], od, G,
                      case["rel_class_weight"], dtype=dtype, grad=grad)
    return seg, r


def matched_rows(od, G, L=1):
    """`Mask2FormerLoss.last["matched"]`-shaped rows [L * sum n_b][4] from od[b] = (queries, objects);
    every layer holds the same rows."""
    goff = np.concatenate([[0], np.cumsum(G)])
    rows = [(l, b, int(q), int(goff[b] + g)) for l in range(L) for b in range(len(od))
            for q, g in zip(od[b][0].tolist(), od[b][1].tolist())]
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)


# ------------------------------------------------------------------------------ case builders
def scores_case(B, R, Q, C1, G, Gr, seed, scale=1.0, od=None):
    """Seeded relation inputs with a planted id assignment: relation k of image b is matched by row
    (3 k + b) % R (k < min(R, Gr)) -- that row's predicate logit and its subject / object id scores
    on the related objects' queries lead by 6 * scale.  od[b] = (queries ascending, their objects);
    default: object g on query (5 g + b) % Q.  The triples of an image are distinct."""
    g = torch.Generator().manual_seed(seed)
    rel = torch.randn(B, R, C1, generator=g) * scale
    sub = torch.randn(B, R, Q, generator=g) * scale
    obj = torch.randn(B, R, Q, generator=g) * scale
    gt_rels, planted, ods = [], [], []
    for b in range(B):
        if od is None:
            qs = [(5 * j + b) % Q for j in range(G[b])]
            assert len(set(qs)) == G[b], "planted queries collide"
            order = np.argsort(qs)
            ods.append((torch.tensor(qs)[order], torch.arange(G[b])[order]))
        else:
            ods.append(od[b])
        a = assigned_queries(G[b], *ods[b])
        seen, rows = set(), []
        while len(rows) < Gr[b]:
            t = (int(torch.randint(0, G[b], (1,), generator=g)), int(torch.randint(0, G[b], (1,), generator=g)),
                 int(torch.randint(1, C1, (1,), generator=g)))
            if t not in seen:
                seen.add(t)
                rows.append(t)
        gr = torch.tensor(rows, dtype=torch.int64)
        n = min(R, Gr[b])
        rs = [(3 * k + b) % R for k in range(n)]
        assert len(set(rs)) == n, "planted rows collide: choose R coprime to 3"
        for k, r in enumerate(rs):
            rel[b, r, gr[k, 2]] += 6.0 * scale
            sub[b, r, a[gr[k, 0]]] += 6.0 * scale
            obj[b, r, a[gr[k, 1]]] += 6.0 * scale
        gt_rels.append(gr)
        planted.append(sorted(zip(rs, range(n))))
    return dict(rel=rel, sub=sub, obj=obj, gt_rels=gt_rels, od=ods, G=list(G), planted=planted,
                rel_class_weight=[0.02] + [1.0] * (C1 - 1))


def full_case(L, B, Q, C, Cr, h, w, Np, G, Gr, seed):
    """A seg_loss_ref.loss_case (R = Q) with relation inputs planted on ITS last-layer matching:
    object j of image b sits on query (3 j + L - 1 + b) % Q there."""
    case = S.loss_case(L, B, Q, C, h, w, Np, G, seed)
    od = []
    for b in range(B):
        pairs = case["planted"][(L - 1, b)]
        od.append((torch.tensor([q for q, _ in pairs]), torch.tensor([j for _, j in pairs])))
    sc = scores_case(B, Q, Q, Cr + 1, G, Gr, seed + 1000, od=od)
    case.update(rel=sc["rel"], sub=sc["sub"], obj=sc["obj"], gt_rels=sc["gt_rels"],
                rel_planted=sc["planted"], rel_class_weight=sc["rel_class_weight"], num_relations=Cr)
    return case


# the cost kernel's shapes (R, Q, Cr + 1, Gr): tiny; one relation; more relations than rows; sizes
# that are no multiple of the wavefront; production.  Image b of a batch has Gr + 2 b relations and
# min(Q, 4 + b) objects; logits of magnitude 30.
COST_SHAPES = [(8, 8, 6, 3), (8, 8, 6, 1), (8, 8, 6, 11), (65, 63, 57, 7), (100, 100, 57, 30)]


def cost_case(R, Q, C1, Gr, B, scale=30.0):
    G = [min(Q, 4 + b) for b in range(B)]
    return scores_case(B, R, Q, C1, G, [Gr + 2 * b for b in range(B)],
                       seed=R * 1000 + Gr * 10 + B, scale=scale)


# id cross-entropy cases through the loss object: (B, R, Q, C1, G, Gr): one matched column (the
# terms and their gradients are exactly 0) beside a general image; every query matched; one
# positive row; sizes that are no multiple of the wavefront with three images
ID_CASES = dict(one_column=(2, 8, 8, 6, (1, 3), (2, 4)), only_one_column=(1, 8, 8, 6, (1,), (3,)),
                all_columns=(1, 8, 8, 6, (8,), (5,)),
                one_row=(2, 8, 8, 6, (3, 4), (1, 1)), odd=(3, 65, 63, 57, (7, 20, 1), (9, 30, 3)),
                more_rels=(1, 8, 8, 6, (4,), (11,)))


def id_case(name):
    B, R, Q, C1, G, Gr = ID_CASES[name]
    return scores_case(B, R, Q, C1, G, Gr, seed=sum(map(ord, name)))


def cost_chain(Q, C1):
    """Roundings of one cost entry as k_rel_id_cost computes it, without the z of the subtraction in
    front of expf (labnotes R17.2): expf 2; the denominator ln n + 2 (its terms' own z and expf,
    weighted by the softmax) + ceil(n / 64) + 5 additions; quotient; weight; the two additions."""
    n = max(Q, C1)
    return int(np.ceil(n / 64) + np.ceil(np.log(n)) + 13)


def id_ce_chain(n, P, B):
    """Roundings of loss_subject_match / loss_object_match (R17.2): the denominator ceil(ln n) +
    ceil(n / 64) + 7 (absolute in log d: needs row magnitudes >= 1), logf 2, + m, - x_t, P serial
    additions, / P, * w, B additions, / B."""
    return int(np.ceil(np.log(max(n, 2))) + np.ceil(n / 64) + P + B + 14)


def id_grad_chain(n):
    """Roundings of one id gradient element without its z (R17.2): expf 2, the denominator
    ceil(ln n) + ceil(n / 64) + 7, quotient, - onehot, the scale's quotient, product."""
    return int(np.ceil(np.log(max(n, 2))) + np.ceil(n / 64) + 13)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_loss.npz")
# the fixture's two cases (tools/make_baseline_loss_golden.py): an image with one object (its id
# terms are exactly 0) beside one with more relations than in the other
FIXTURE_CASES = dict(a=dict(L=2, B=2, Q=8, C=5, Cr=6, h=13, w=21, Np=50, G=(3, 2), Gr=(4, 2), seed=31),
                     b=dict(L=2, B=2, Q=8, C=5, Cr=6, h=13, w=21, Np=50, G=(1, 4), Gr=(1, 6), seed=32))


def golden_case(name):
    """Fixture case -> (a full_case-shaped dict, the stored reference values)."""
    z = np.load(GOLDEN)
    pre = name + "."
    L, B, Q, C, Cr, h, w, Np = (int(v) for v in z[pre + "shape"])
    T = lambda k: torch.from_numpy(z[pre + k])
    case = dict(cls=T("cls"), mask=T("mask"), gt_labels=[T("gt_labels.%d" % b) for b in range(B)],
                gt_masks=[T("gt_masks.%d" % b) for b in range(B)], num_classes=C, num_points=Np,
                class_weight=[1.0] * C + [0.1], num_relations=Cr,
                rel_class_weight=[0.02] + [1.0] * Cr, rel=T("rel"), sub=T("sub"), obj=T("obj"),
                gt_rels=[T("gt_rels.%d" % b) for b in range(B)],
                points=dict(assign=[[T("assign.%d.%d" % (l, b)) for b in range(B)] for l in range(L)],
                            candidates=[T("candidates.%d" % l) for l in range(L)],
                            tail=[T("tail.%d" % l) for l in range(L)]))
    ref = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    return case, ref


# ------------------------------------------------------------------------------ the reference itself
def load_reference():
    """The reference's CrossHeadBaseline class with the names its module bound at import (to the
    inference stubs) replaced in ITS namespace; the id assigner and MultilabelCrossEntropy are the
    reference's own (matcher.py, losses/seg_losses.py), registered by oracle.ref_shim."""
    from oracle import mmdet_train as T
    S.load_reference()           # (install_training + the reference's point_sample.py)
    mod = sys.modules["pairnet.models.relation_heads.baseline"]
    ps = sys.modules["pairnet.models.panoptic_heads.point_sample"]
    mod.__dict__.update(
        point_sample=T.point_sample, multi_apply=T.multi_apply, reduce_mean=lambda t: t,
        get_uncertain_point_coords_with_randomness=ps.get_uncertain_point_coords_with_randomness)
    return mod.CrossHeadBaseline


def run_reference(case, dtype=torch.float32, cfg=None, rel_cfg=None):
    """`CrossHeadBaseline.loss` of the reference on a full_case -> (the 30-key loss dict, d sum of
    the THREE relation terms / d (rel, subject_scores, object_scores), d sum of all / d cls), in
    `dtype`.  (The segmentation terms do not depend on the relation logits, so the gradient of the
    sum of all 30 with respect to them is the gradient of the three.)"""
    from oracle import mmdet_train as T
    cfg, rel_cfg = cfg or S.CFG, rel_cfg or REL_CFG
    Head = load_reference()
    head = Head.__new__(Head)
    L, B, Q = case["cls"].shape[:3]
    Np = case["num_points"]
    cw = [float(np.float32(v)) for v in case["class_weight"]]
    rcw = [float(np.float32(v)) for v in case["rel_class_weight"]]
    MCE = sys.modules["pairnet.models.losses.seg_losses"].MultilabelCrossEntropy
    cc = lambda w: dict(type="ClassificationCost", weight=w)
    attrs = dict(num_points=Np, num_queries=Q, num_classes=case["num_classes"], class_weight=cw,
                 rel_class_weight=rcw, rel_cls_out_channels=case["num_relations"] + 1,
                 oversample_ratio=cfg["oversample_ratio"],
                 importance_sample_ratio=cfg["importance_sample_ratio"],
                 mask_assigner=T.build_assigner(dict(
                     type="MaskHungarianAssigner", cls_cost=cc(cfg["c_cls"]),
                     mask_cost=dict(type="CrossEntropyLossCost", weight=cfg["c_mask"], use_sigmoid=True),
                     dice_cost=dict(type="DiceCost", weight=cfg["c_dice"], pred_act=True,
                                    eps=cfg["c_dice_eps"]))),
                 id_assigner=T.build_assigner(dict(
                     type="OldIdMatcher", sub_id_cost=cc(rel_cfg["c_sub"]),
                     obj_id_cost=cc(rel_cfg["c_obj"]), r_cls_cost=cc(rel_cfg["c_rel"]))),
                 sampler=T.build_sampler(dict(type="MaskPseudoSampler")),
                 loss_cls=T.CrossEntropyLoss(use_sigmoid=False, loss_weight=cfg["w_cls"],
                                             reduction="mean", class_weight=cw),
                 loss_mask=S.SigmoidCE(cfg["w_mask"]), loss_dice=S.DiceLoss(cfg["w_dice"], cfg["dice_eps"]),
                 rel_loss_cls=T.CrossEntropyLoss(use_sigmoid=False, loss_weight=rel_cfg["w_rel"],
                                                 reduction="mean", class_weight=rcw),
                 sub_id_loss=MCE(loss_weight=rel_cfg["w_sub"]),
                 obj_id_loss=MCE(loss_weight=rel_cfg["w_obj"]))
    for k, v in attrs.items():
        object.__setattr__(head, k, v)
    pts, G = case["points"], [int(g.shape[0]) for g in case["gt_labels"]]
    Ml = sum(min(Q, g) for g in G)
    k = int(cfg["importance_sample_ratio"] * Np)
    draws = []
    for l in range(L):        # the order of the reference's torch.rand calls
        draws += [pts["assign"][l][b].reshape(1, -1, 2) for b in range(B)]
        if Ml:
            draws.append(pts["candidates"][l])
            if k < Np:
                draws.append(pts["tail"][l])
    V = lambda t: t.detach().clone().to(dtype).requires_grad_(True)
    cls, mask, rel, sub, obj = (V(case[n]) for n in ("cls", "mask", "rel", "sub", "obj"))
    R, h, w = rel.shape[1], mask.shape[-2], mask.shape[-1]
    seg = torch.zeros(B, R, h, w, dtype=dtype)       # (sub_seg / obj_seg: only their shape is read)
    real_float = torch.Tensor.float
    if dtype == torch.float64:       # the reference's `.float()` casts follow the run's precision
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        with S.injected_rand(draws, dtype):
            out = head.loss(dict(cls=cls, rel=rel, subject_scores=sub, object_scores=obj),
                            dict(mask=mask, sub_seg=seg, obj_seg=seg),
                            [g.long() for g in case["gt_rels"]], None,
                            [g.long() for g in case["gt_labels"]],
                            [m.to(dtype) for m in case["gt_masks"]], [dict() for _ in range(B)])
    finally:
        torch.Tensor.float = real_float
    sum(out.values()).backward()
    return ({k: v.detach() for k, v in out.items()}, (rel.grad.detach(), sub.grad.detach(),
                                                      obj.grad.detach()), cls.grad.detach())
