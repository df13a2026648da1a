"""CPU: the odd pyramids of tests/grad_shapes.py are what they claim (every condition the GPU tests
of the tapes rest on, from `oracle.seeded.seeded_feats` and the tapes' own size arithmetic), and the
float64 statements the tapes are measured against -- tests/fpn_grad_ref.py, tests/seg_grad_ref.py,
tests/rel_grad_ref.py, tests/tri_grad_ref.py -- agree with float64 autograd through the
reference-pinned oracles at size A (52 x 76: 13 x 19 over 7 x 10, 4 x 5, 2 x 3), as the `*_refs.py`
files show at 64 x 96.  A reference is proven at a shape before a kernel is measured against it."""
import pytest
import torch
import torch.nn.functional as F

import fpn_grad_ref as FR
import grad_shapes as GS
import rel_grad_ref as RR
import seg_grad_ref as SR
import tri_grad_ref as TR
from helpers import baseline_cfg, oracle_baseline_head, oracle_psgtr2_head
from oracle import seeded
from oracle.baseline_head import OracleCrossHeadBaseline
from oracle.psgtr_head2 import OraclePSGTrHead2

A = GS.A
_S = {}


# ------------------------------------------------------------------------------ the shapes
def test_the_shapes_cover_what_they_claim():
    pyr = {s.name: GS.pyramid(s.H, s.W) for s in GS.IMAGE_SHAPES + [GS.OLD]}
    for s in GS.IMAGE_SHAPES + [GS.OLD]:              # the restated arithmetic is the pyramid's
        feats = seeded.seeded_feats(1, 1, s.H, s.W, channels=(1, 1, 1, 1))
        assert [tuple(f.shape[-2:]) for f in feats] == pyr[s.name], s.name
    assert pyr["A"] == [(13, 19), (7, 10), (4, 5), (2, 3)]
    assert pyr["B"] == [(18, 25), (9, 13), (5, 7), (3, 4)]
    assert pyr["C"] == [(16, 22), (8, 11), (4, 6), (2, 3)]
    ab = pyr["A"] + pyr["B"]
    # every level of A and of B has an odd side, on both axes somewhere
    assert all(h % 2 or w % 2 for h, w in ab)
    assert sum(1 for h, w in ab if h % 2) >= 2 and sum(1 for h, w in ab if w % 2) >= 2
    assert sum(1 for h, w in ab if h % 2 and not w % 2) >= 1
    assert sum(1 for h, w in ab if w % 2 and not h % 2) >= 1
    # ceil and floor differ at each of the backbone's stride-2 steps, somewhere in A u B
    for l in range(3):
        assert any(GS.step(n) != n // 2 for s in ("A", "B") for n in pyr[s][l]), l
    assert all(GS.floor_pyramid(s.H, s.W) != pyr[s.name] for s in GS.TAPE_SHAPES)
    # ... and at none of them in what the tapes were checked at before
    assert GS.floor_pyramid(GS.OLD.H, GS.OLD.W) == pyr["64x96"]
    for s in GS.TAPE_SHAPES:
        h, w = pyr[s.name][0]
        assert (s.B * h * w) % 64 != 0, s.name                       # C2 rows: a ragged last tile
    assert GS.encoder_tokens(GS.B) == 117 + 35 + 12 == 164 and GS.encoder_tokens(GS.B) % 32 != 0
    assert GS.B.B % 2 == 1
    counts = [n for s in GS.TAPE_SHAPES for n in GS.key_counts(s)]
    assert GS.key_counts(A) == [6, 20, 70] and GS.key_counts(GS.B) == [12, 35, 117]
    assert any(n > 64 and n % 32 for n in counts)                    # mask bits: a ragged last word
    assert all(n % 32 for n in counts)
    assert any(pyr[s.name][0][1] % 4 for s in GS.TAPE_SHAPES)         # mask-feature row width
    assert GS.C.H % 2 == 1 and GS.C.W % 2 == 1
    assert GS.gt_mask_size(GS.C) == (30, 43) and GS.gt_mask_size(A) == (26, 38)
    # at C the ground-truth masks are not the mask feature's size times two either
    assert GS.gt_mask_size(GS.C) != (2 * pyr["C"][0][0], 2 * pyr["C"][0][1])
    for s in GS.IMAGE_SHAPES:
        assert len(s.counts) == s.B and len(GS.metas(s)) == s.B


# ------------------------------------------------------------------------------ FPN branch
def _pd():
    if "pd" not in _S:
        head, _, _ = oracle_baseline_head(1234)
        _S["pd"] = head.double().pixel_decoder
    return _S["pd"]


def test_fpn_branch_statement_and_its_gradient_at_A():
    """Value and every gradient of the branch statement against autograd through the oracle's own
    pixel decoder (which holds the branch as modules) at 13 x 19 over 7 x 10."""
    pd = _pd()
    for p in pd.parameters():
        p.requires_grad_(True)
        p.grad = None
    feats = [f.double().requires_grad_() for f in seeded.seeded_feats(99, A.B, A.H, A.W)]
    mf, outs = pd(feats)
    assert tuple(mf.shape[-2:]) == (13, 19) and tuple(outs[2].shape[-2:]) == (7, 10)
    G = torch.randn(mf.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    p = FR.branch_params(pd)
    names = list(p)
    ref = torch.autograd.grad((mf * G).sum(), [feats[0]] + [p[n] for n in names], retain_graph=True)
    c2 = feats[0].detach().requires_grad_()
    mem2 = outs[2].detach().requires_grad_()
    mine, z = FR.branch(c2, mem2, p, baseline_cfg()["pixel_decoder"]["norm_cfg"]["num_groups"])
    assert float((mine - mf).detach().abs().max()) <= 1e-12
    got = torch.autograd.grad((mine * G).sum(), [c2] + [p[n] for n in names] + [mem2])
    for n, a, b in zip(["C2"] + names, got, ref):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), n
    # the gradient handed to the finest memory level is the adjoint statement of the upsampling
    y_grad = torch.autograd.grad(
        (F.interpolate(mem2, size=(13, 19), mode="bilinear", align_corners=False) * G).sum(), mem2)[0]
    d, mag, extra = FR.bilinear_adjoint(G, 7, 10)
    assert float((d - y_grad).abs().max()) <= 1e-12
    assert float(got[-1].abs().max()) > 0
    for p_ in pd.parameters():
        p_.requires_grad_(False)


@pytest.mark.parametrize("hi,wi,ho,wo", [(7, 10, 13, 19), (9, 13, 18, 25), (8, 11, 16, 22)])
def test_bilinear_adjoint_statement_at_the_odd_pairs(hi, wi, ho, wo):
    g = torch.Generator().manual_seed(hi + wo)
    x = torch.randn(2, 3, hi, wi, generator=g, dtype=torch.float64, requires_grad=True)
    G = torch.randn(2, 3, ho, wo, generator=g, dtype=torch.float64)
    ref, = torch.autograd.grad(F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=False),
                               x, G)
    d, mag, extra = FR.bilinear_adjoint(G, hi, wi)
    assert float((d - ref).abs().max()) <= 1e-12
    assert bool((mag >= d.abs() - 1e-12).all()) and bool((extra >= 0).all())


@pytest.mark.parametrize("hw", [13 * 19, 18 * 25])
def test_group_norm_backward_statement_on_the_odd_planes(hw):
    g = torch.Generator().manual_seed(hw)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, gamma, beta, dy = rn(2, hw, 256).requires_grad_(), rn(256).requires_grad_(), \
        rn(256).requires_grad_(), rn(2, hw, 256)
    y = F.group_norm(x.permute(0, 2, 1), 32, gamma, beta, 1e-5).permute(0, 2, 1)
    dx, dg, db = torch.autograd.grad(F.relu(y), (x, gamma, beta), dy)
    s = FR.group_norm_bwd(x.detach(), dy, gamma.detach(), 32, 1e-5, (y.detach() > 0).double())
    for k, ref in (("dx", dx), ("dgamma", dg), ("dbeta", db)):
        assert float((s[k] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), k


# ------------------------------------------------------------------------------ segmenter heads
def _keep(store, t):
    """A forward hook's body: keep an intermediate and its gradient; None leaves the output alone."""
    t.retain_grad()
    store(t)


def _baseline_run():
    """One float64 run of the oracle baseline head's own forward at A with autograd on; every
    decoder layer's output queries and the mask feature captured by hooks."""
    if "baseline" not in _S:
        head_o, sd, _ = oracle_baseline_head(1234)
        head_o = head_o.double()
        for p in head_o.parameters():
            p.requires_grad_(True)
        feats = [f.double() for f in seeded.seeded_feats(99, A.B, A.H, A.W)]
        seen = dict(q=[])
        hooks = [l.register_forward_hook(lambda m, i, o: _keep(seen["q"].append, o))
                 for l in head_o.transformer_decoder.layers]
        hooks.append(head_o.pixel_decoder.register_forward_hook(
            lambda m, i, o: _keep(lambda t: seen.__setitem__("mf", t), o[0])))
        cls, masks = OracleCrossHeadBaseline.forward.__wrapped__(head_o, feats, GS.metas(A))
        for h in hooks:
            h.remove()
        _S["baseline"] = (head_o, feats, cls, masks, seen)
    return _S["baseline"]


def _compact_grads(L, B, Q, nc, hw, counts, seed):
    g = torch.Generator().manual_seed(seed)
    g_cls = torch.randn(L, B, Q, nc, generator=g, dtype=torch.float64)
    rows = torch.cat([torch.randperm(Q, generator=g)[:n].sort()[0] + (l * B + b) * Q
                      for l in range(L) for b, n in enumerate(counts)]).long()
    rows[1] = -1                                          # one failed row
    return g_cls, torch.randn(rows.numel(), hw[0], hw[1], generator=g, dtype=torch.float64), rows


def test_segmenter_statement_and_its_gradient_at_A():
    """`seg_grad_ref.heads` reproduces the oracle's class and mask stacks at 13 x 19, and
    `seg_grad_ref.vjp` is autograd of the same functional through the oracle's own forward: the ten
    head parameters, the mask feature and the last layer's queries (what nothing downstream adds to:
    the attention masks are detached thresholds)."""
    head_o, feats, cls, masks, seen = _baseline_run()
    cls_o, mask_o = cls["cls"], masks["mask"]
    L, B, Q, nc = cls_o.shape
    assert (L, B, Q) == (9, A.B, 100) and tuple(mask_o.shape[-2:]) == (13, 19)
    q_all = torch.stack([q.transpose(0, 1) for q in seen["q"]]).detach()
    MF = seen["mf"].detach().flatten(2).transpose(1, 2)
    P = {k: v.detach() for k, v in head_o.named_parameters()}
    c, m, _ = SR.heads(q_all, MF, P)
    cd, md = cls_o.detach(), mask_o.detach()
    assert float((c - cd).abs().max()) <= 1e-12 * max(1.0, float(cd.abs().max()))
    assert float((m.view(md.shape) - md).abs().max()) <= 1e-12 * max(1.0, float(md.abs().max()))
    g_cls, g_mask, rows = _compact_grads(L, B, Q, nc, (13, 19), A.counts, seed=7)
    head_o.zero_grad(set_to_none=True)
    for t in seen["q"] + [seen["mf"]]:
        t.grad = None
    SR.functional(cls_o, mask_o.flatten(3), g_cls, g_mask, rows).backward(retain_graph=True)
    got = SR.vjp(q_all, MF, P, g_cls, g_mask, rows)
    named = dict(head_o.named_parameters())
    rel = lambda a, b: float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
    for k in SR.HEAD_PARAMS:
        assert rel(got[k], named[k].grad) <= 1e-12, k
    assert rel(got["MF"], seen["mf"].grad.flatten(2).transpose(1, 2)) <= 1e-12
    assert rel(got["q"][8], seen["q"][8].grad.transpose(0, 1)) <= 1e-12
    assert float(got["MF"].abs().max()) > 0


# ------------------------------------------------------------------------------ relation stage
def test_relation_statement_and_its_gradient_at_A():
    """`rel_grad_ref.relation_stage` equals the oracle forward's three relation outputs at the 6 /
    20 / 70-key levels, and autograd through it gives the oracle forward's own gradients for every
    parameter of the relation branch."""
    head_o, feats, cls, masks, seen = _baseline_run()
    with torch.no_grad():
        mem, q, level = RR.trunk(head_o, feats)
        assert level[2] == GS.key_counts(A) and level[0] == [(2, 3), (4, 5), (7, 10)]
        rel, sub, obj = RR.relation_stage(head_o, mem, q, *level)
    for name, got in (("rel", rel), ("subject_scores", sub), ("object_scores", obj)):
        assert got.shape == cls[name].shape
        assert float((got - cls[name].detach()).abs().max()) <= 1e-12, name
    assert float((q - seen["q"][8].detach().transpose(0, 1)).abs().max()) <= 1e-12
    g = torch.Generator().manual_seed(0)                       # (`reached` draws in this order)
    draw = lambda t: torch.randn(t.shape, generator=g, dtype=t.dtype)
    gs = [draw(rel), draw(sub), draw(obj)]
    head_o.zero_grad(set_to_none=True)
    RR.functional(cls["rel"], cls["subject_scores"], cls["object_scores"], *gs).backward(
        retain_graph=True)
    ref = {k: p.grad.clone() for k, p in head_o.named_parameters()
           if p.grad is not None and k.startswith(RR.REL_PREFIXES)}
    grads, dmem, dq = RR.reached(head_o, mem, q, level, seed=0)
    assert set(ref) == {k for k in grads if k.startswith(RR.REL_PREFIXES)} and len(ref) == 120
    for k, r in ref.items():
        assert float((grads[k] - r).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max())), k
    assert float(dmem.abs().max()) > 0 and float(dq.abs().max()) > 0
    head_o.zero_grad(set_to_none=True)


# ------------------------------------------------------------------------------ triplet heads
def test_triplet_statement_and_its_gradient_at_A():
    """`tri_grad_ref.heads` equals the oracle `PSGTrHead2`'s five outputs at A, and autograd of
    `tri_grad_ref.functional` through it equals autograd of the same functional through the oracle's
    own forward: head parameters, mask feature, last queries."""
    head_o, sd, _ = oracle_psgtr2_head(1234)
    head_o = head_o.double()
    for p in head_o.parameters():
        p.requires_grad_(True)
    feats = [f.double() for f in seeded.seeded_feats(99, A.B, A.H, A.W)]
    seen = {}
    h1 = head_o.transformer_decoder.layers[-1].register_forward_hook(
        lambda m, i, o: _keep(lambda t: seen.__setitem__("q", t), o))
    h2 = head_o.pixel_decoder.register_forward_hook(
        lambda m, i, o: _keep(lambda t: seen.__setitem__("MF", t), o[0]))
    try:
        cls, masks = OraclePSGTrHead2.forward.__wrapped__(head_o, feats, GS.metas(A))
    finally:
        h1.remove()
        h2.remove()
    Bn, Q = A.B, cls["sub"].shape[2]
    assert tuple(masks["sub_seg"].shape[-2:]) == (13, 19)
    gen = torch.Generator().manual_seed(9)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    rows = torch.cat([torch.randperm(Q, generator=gen)[:n].sort()[0] + b * Q
                      for b, n in enumerate((3, 1))]).long()
    g = [rn(Bn, Q, cls["sub"].shape[-1]), rn(Bn, Q, cls["obj"].shape[-1]),
         rn(Bn, Q, cls["rel"].shape[-1]), rn(4, 13, 19), rn(4, 13, 19)]
    oracle_out = (cls["sub"][0], cls["obj"][0], cls["rel"][0], masks["sub_seg"][0].flatten(2),
                  masks["obj_seg"][0].flatten(2))
    TR.functional(oracle_out, *g, rows).backward()
    named = dict(head_o.named_parameters())
    ref = {k: named[k].grad.clone() for k in TR.HEAD_PARAMS}
    ref_q, ref_MF = seen["q"].grad.transpose(0, 1), seen["MF"].grad.flatten(2).transpose(1, 2)
    p = {k: v.detach().clone().requires_grad_() for k, v in named.items() if k in TR.HEAD_PARAMS}
    qf = named["query_feat.weight"].detach()
    q = seen["q"].detach().transpose(0, 1).clone().requires_grad_()
    MF = seen["MF"].detach().flatten(2).transpose(1, 2).clone().requires_grad_()
    out = TR.heads(q, qf, MF, p)
    for name, a, b in zip(("sub", "obj", "rel", "sub_seg", "obj_seg"), out, oracle_out):
        assert float((a.detach() - b.detach()).abs().max()) <= 1e-12, name
    TR.functional(out, *g, rows).backward()
    rel = lambda a, b: float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
    for k in TR.HEAD_PARAMS:
        assert rel(p[k].grad, ref[k]) <= 1e-12, k
    assert rel(q.grad, ref_q) <= 1e-12 and rel(MF.grad, ref_MF) <= 1e-12
    assert float(MF.grad.abs().max()) > 0
