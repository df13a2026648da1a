"""GPU: `BaselineHeadGrad` (pair-net_amd/seg_grad.py) -- all six logit gradients of
`CrossHeadBaseline.full_losses` carried through the relation branch and, with its share added,
through the class / mask heads and the nine masked decoder layers -- against float64 autograd: the
relation stage through the statement of tests/rel_grad_ref.py (the oracle's own layer modules), the
heads through tests/seg_grad_ref.py, the masked decoder through the oracle's layers under the tape's
mask bits (as tests/test_seg_grad_gpu.py does it).  Tolerance: 1e-4 of each tensor's largest entry;
the taped forward reproduces the plan's relation outputs to 1e-4 absolute.  A seeded
`CrossHeadBaseline` at the 64 x 96 pyramid, `return_all_layers=True`, two images with 3 and 5
objects."""
import numpy as np
import pytest
import torch

import dropout_ref
import fpn_grad_ref as FR
import rel_grad_ref as RR
import seg_grad_ref as R
from helpers import baseline_cfg, oracle_baseline_head
from oracle import seeded
from test_grad_gpu import _compare, _compare_params, _fp32_miss, _print, _unpack_mask
from test_seg_grad_gpu import COUNTS, _oracle64, _random_grads, _train_cfg, _trunk_names

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 64, 96
_S = {}


def _setup():
    """(head, sd, cls, masks, pl, device feats) of one `return_all_layers=True` forward."""
    if "head" not in _S:
        assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
        from pairnet_amd import CrossHeadBaseline
        _, sd, _ = oracle_baseline_head(1234)
        cc = lambda w: dict(type="ClassificationCost", weight=w)
        tc = dict(_train_cfg(), id_assigner=dict(type="OldIdMatcher", sub_id_cost=cc(1.0),
                                                 obj_id_cost=cc(1.0), r_cls_cost=cc(1.0)))
        head = CrossHeadBaseline(**baseline_cfg(), train_cfg=tc)
        head.load_state_dict(sd)
        head.to(DEV)
        head.exact_mask_order = True
        head.return_all_layers = True
        feats = [f.to(DEV) for f in seeded.seeded_feats(99, 2, H, W)]
        metas = [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)] * 2
        cls, masks = head.forward(feats, metas)
        torch.cuda.synchronize()
        _S["head"] = (head, sd, cls, masks, head._last_plan, feats)
    return _S["head"]


def _tape():
    if "tape" not in _S:
        from pairnet_amd import BaselineHeadGrad
        head, _, _, _, pl, _ = _setup()
        tape = BaselineHeadGrad(head)
        _S["tape"] = (tape, tape.forward_from_plan(pl, with_mask=True))
    return _S["tape"]


def _rel_grads(seed, zero=False):
    g = torch.Generator().manual_seed(seed)
    draw = (lambda *s: torch.zeros(*s)) if zero else (lambda *s: torch.randn(*s, generator=g))
    return dict(rel=draw(2, 100, 57).to(DEV), subject_scores=draw(2, 100, 100).to(DEV),
                object_scores=draw(2, 100, 100).to(DEV))


def _zero_seg_grads(pl):
    g = _random_grads(9, 2, 100, 134, pl.hw2, COUNTS, seed=1, zero_layers=range(9))
    g["mask"].zero_()
    assert float(g["cls"].abs().max()) == 0.0 and int(g["mask_rows"].max()) == -1
    return g


def _branch_names():
    from pairnet_amd import BaselineHeadGrad, SegmenterHeadGrad
    head = _setup()[0]
    groups = BaselineHeadGrad.param_groups(head)
    return [n for _, names in groups[:len(groups) - len(SegmenterHeadGrad.param_groups(head))]
            for n in names]


def _all_names():
    return _branch_names() + _trunk_names()


class _FixedDrop(torch.nn.Module):
    """Stands in for an nn.Dropout of the oracle: multiplies with keep / (1 - p), sequence-first."""

    def __init__(self, mult):
        super().__init__()
        self.mult = mult

    def forward(self, x):
        return x * self.mult


def _reference(tape, pl, sd, grads, drop=None, dtype=torch.float64):
    """Float64 autograd of the linear functional the six gradients define, through the oracle's
    nine masked layers (under the tape's mask bits), the statement's heads and the relation stage
    -> (d mem, d MF, oracle head with .grad, (rel, sub, obj) values)."""
    head_o = _oracle64(sd).to(dtype)        # (`dtype`: fp32 for the oracle's own miss, `_fp32_miss`)
    B, Q = pl.B, tape.Q
    if drop is not None:
        s = float(dropout_ref.scale(drop.p))
        for i, layer in enumerate(head_o.relation_decoder.layers):
            ffn = layer.ffns[0]
            assert isinstance(ffn.layers[0][2], torch.nn.Dropout) and \
                isinstance(ffn.layers[2], torch.nn.Dropout)
            mult = []
            for which, C in ((0, tape.head.rel_ffn), (1, 256)):
                keep = dropout_ref.keep_mask(B * Q * C, drop.p, drop.seed, drop.subseq, drop.step,
                                             2 * i + which)
                mult.append(torch.from_numpy(np.asarray(keep)).view(B, Q, C).permute(1, 0, 2)
                            .double() * s)
            ffn.layers[0][2] = _FixedDrop(mult[0])
            ffn.layers[2] = _FixedDrop(mult[1])
    mem = pl.X.cpu().to(dtype).requires_grad_()
    MF = pl.MF.view(B, pl.HW2, 256).cpu().to(dtype).requires_grad_()
    keys, key_pos = RR.keys_of(head_o, mem, pl.shapes, pl.start, pl.N)
    q = head_o.query_feat.weight.unsqueeze(1).repeat((1, B, 1))
    q_pos = head_o.query_embed.weight.unsqueeze(1).repeat((1, B, 1))
    qs = []
    for i, layer in enumerate(head_o.transformer_decoder.layers):
        s = tape.dt["layers"][i]
        l = i % 3
        mask = _unpack_mask(s["bits"], s["rowall"], B, Q, pl.N[l])
        mask = mask.unsqueeze(1).repeat((1, head_o.n_heads, 1, 1)).flatten(0, 1)
        q = layer(query=q, key=keys[l], value=keys[l], query_pos=q_pos, key_pos=key_pos[l],
                  attn_masks=[mask, None], query_key_padding_mask=None, key_padding_mask=None)
        qs.append(q.transpose(0, 1))
    cls, mask, _ = R.heads(torch.stack(qs), MF, dict(head_o.named_parameters()))
    rel, sub, obj = RR.relation_stage(head_o, mem, qs[-1], pl.shapes, pl.start, pl.N)
    d = lambda k: grads[k].cpu().to(dtype)
    total = R.functional(cls, mask, d("cls"), d("mask"), grads["mask_rows"].cpu()) + \
        RR.functional(rel, sub, obj, d("rel"), d("subject_scores"), d("object_scores"))
    total.backward()
    return mem.grad, MF.grad, head_o, (rel.detach(), sub.detach(), obj.detach())


def _compare_all(pl, dmem, dMF, g, ref, report, names, ref32=None):
    """`ref32`: `_reference(..., dtype=torch.float32)` -- the bounds then follow `_compare`'s `e32`."""
    dmem_ref, dMF_ref, head_o = ref[:3]
    lv = lambda t: {"memory tokens of level %d" % l: t[:, pl.start[l]:pl.start[l] + pl.N[l]]
                    for l in range(3)}
    e32 = None
    if ref32 is not None:
        e32 = _fp32_miss(dict(lv(dmem_ref), **{"mask feature": dMF_ref}),
                         dict(lv(ref32[0]), **{"mask feature": ref32[1]}), head_o, ref32[2])
    for l in range(3):
        a, b = pl.start[l], pl.start[l] + pl.N[l]
        _compare("memory tokens of level %d" % l, dmem[:, a:b], dmem_ref[:, a:b], report, e32)
    _compare("mask feature", dMF, dMF_ref, report, e32)
    _compare_params(g, head_o, report, names, e32)


def test_taped_forward_equals_the_plans_relation_outputs():
    head, _, cls, _, pl, _ = _setup()
    tape, out = _tape()
    torch.cuda.synchronize()
    for k, shape in (("rel", (2, 100, 57)), ("subject_scores", (2, 100, 100)),
                     ("object_scores", (2, 100, 100))):
        assert out[k].shape == cls[k].shape == shape
        err = float((out[k] - cls[k]).abs().max())
        print("taped %s: %.2e (max |.| %.2f)" % (k, err, float(cls[k].abs().max())))
        assert err < 1e-4
    assert out["cls"].shape == (9, 2, 100, 134) and "mask" in out


@pytest.mark.parametrize("algo", ["keysplit", "mha_bwd"])
def test_relation_branch_alone(algo):
    head, sd, _, _, pl, _ = _setup()
    tape, _ = _tape()
    grads = dict(_zero_seg_grads(pl), **_rel_grads(41))
    keep = tape.attn_bwd_algo
    tape.attn_bwd_algo = algo
    try:
        dmem, dMF, g = tape.backward(grads, counts=COUNTS)
    finally:
        tape.attn_bwd_algo = keep
    torch.cuda.synchronize()
    if "alone" not in _S:
        _S["alone"] = _reference(tape, pl, sd, grads)
    report = []
    _compare_all(pl, dmem, dMF, g, _S["alone"], report, _all_names())
    _print(report)
    assert float(dMF.abs().max()) == 0.0
    assert sorted(g) == sorted(_all_names())
    assert float(tape.dq_rel.abs().max()) > 0
    for n in ("rel_query_feat.weight", "relation_decoder.layers.0.attentions.0.attn.in_proj_weight",
              "transformer_decoder.layers.0.ffns.0.layers.1.weight", "query_embed.weight"):
        assert float(g[n].abs().max()) > 0, n


def _own_losses():
    head, _, cls, masks, pl, _ = _setup()
    gen = torch.Generator().manual_seed(8)
    gt_labels = [torch.randint(0, 133, (n,), generator=gen) for n in COUNTS]
    gt_masks = [(torch.rand(n, 32, 48, generator=gen) > 0.6).to(torch.uint8) for n in COUNTS]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 0, 17], [1, 2, 55]]),
               torch.tensor([[0, 4, 2], [3, 1, 30], [4, 2, 9], [1, 0, 41]])]
    grads = {}
    losses = head.full_losses(cls, masks, gt_rels, None, gt_labels, gt_masks, [dict()] * 2,
                              grads=grads, seed=3)
    assert len(losses) == 30 and sorted(grads) == sorted(
        ("cls", "mask", "mask_rows", "rel", "subject_scores", "object_scores"))
    assert head._seg_loss.last["counts"] == COUNTS
    return grads


def test_all_six_gradients_from_the_heads_own_losses():
    head, sd, _, _, pl, _ = _setup()
    tape, _ = _tape()
    grads = _own_losses()
    ends = []
    dmem, dMF, g = tape.backward(grads, on_ready=ends.append, counts=COUNTS)
    torch.cuda.synchronize()
    ref = _reference(tape, pl, sd, grads)
    report = []
    _compare_all(pl, dmem, dMF, g, ref, report, _all_names())
    _print(report)
    assert set(g) == {k for k, p in ref[2].named_parameters() if p.grad is not None}
    assert set(g) == {k for k in head.param_shapes() if not k.startswith("pixel_decoder.")} - \
        set(RR.UNREACHABLE)
    # flat layout: views of one buffer, the new groups first, on_ready ends monotone
    lo = tape.flat_grad.data_ptr()
    for n, (off, shape, numel) in tape.layout.items():
        assert g[n].data_ptr() == lo + 4 * off and tuple(g[n].shape) == shape and off % 64 == 0
    assert ends == sorted(ends) and ends[-1] == tape.flat_numel == tape.size_of(head)
    assert ends[0] == tape.group_end["rel_cls_embed"] and list(tape.layout)[:2] == _branch_names()[:2]
    # two backward calls on one tape: the same bits
    kept = (dmem.clone(), dMF.clone(), tape.flat_grad.clone())
    dmem2, dMF2, _ = tape.backward(grads, counts=COUNTS)
    assert torch.equal(dmem2, kept[0]) and torch.equal(dMF2, kept[1])
    assert torch.equal(tape.flat_grad, kept[2])
    # the head's convenience returns the same triple, and seg_backward keeps its meaning
    dmem3, dMF3, g3 = head.head_backward(grads)
    torch.cuda.synchronize()
    assert torch.equal(dmem3, kept[0]) and torch.equal(dMF3, kept[1]) and sorted(g3) == sorted(g)
    assert all(torch.equal(g3[k], kept[2][o:o + n].view(s)) for k, (o, s, n) in tape.layout.items())
    _, _, g_seg = head.seg_backward(grads)
    assert sorted(g_seg) == sorted(_trunk_names())


def test_zero_relation_gradients_give_the_parents_bits():
    from pairnet_amd import SegmenterHeadGrad
    head, _, _, _, pl, _ = _setup()
    tape, _ = _tape()
    grads = _random_grads(9, 2, 100, 134, pl.hw2, COUNTS, seed=21)
    parent = SegmenterHeadGrad(head)
    parent.forward_from_plan(pl)
    pm, pF, pg = parent.backward(grads, counts=COUNTS)
    dmem, dMF, g = tape.backward(dict(grads, **_rel_grads(0, zero=True)), counts=COUNTS)
    torch.cuda.synchronize()
    assert torch.equal(dmem, pm) and torch.equal(dMF, pF)
    for k in pg:
        assert torch.equal(g[k], pg[k]), k
    assert sorted(set(g) - set(pg)) == sorted(_branch_names())
    for k in _branch_names():
        assert float(g[k].abs().max()) == 0.0, k
    assert float(pg["level_embed.weight"].abs().max()) > 0


def test_through_the_pixel_decoder():
    """`full_backward` against float64: the head's reference gradients (d mem, d MF) carried on by
    autograd through the oracle's pixel decoder, the FPN branch under the tape's own ReLU gate (as
    tests/test_fpn_grad_gpu.py does it).  Nothing here is compared bit for bit: the walk behind the
    first `pn_msda_bwd_f32` is not reproducible (labnotes R20.3)."""
    head, sd, cls, masks, pl, feats = _setup()
    tape, _ = _tape()
    grads = _own_losses()
    dfeats, g = head.full_backward(grads, feats, pl=pl, need_dc2=True)
    torch.cuda.synchronize()
    dmem_ref, dMF_ref, head_o, _ = _reference(tape, pl, sd, grads)
    head_grads = {k: p.grad.clone() for k, p in head_o.named_parameters() if p.grad is not None}
    pd = head_o.pixel_decoder
    f64 = [f.cpu().double().requires_grad_() for f in feats]
    _, memories = pd(f64)
    mem_ref = torch.cat([m.flatten(2).transpose(1, 2) for m in memories], 1)
    gate = (head._segpd_tape.t["fpn"]["Y"] > 0).permute(0, 3, 1, 2).cpu().double()
    MFr, z = FR.branch(f64[0], memories[2], FR.branch_params(pd), head.gn_groups, gate=gate)
    assert FR.gate_mismatch(gate, z.detach()) <= FR.GATE_CAP
    MFr = MFr.flatten(2).transpose(1, 2)
    names = [n for n, _ in head_o.named_parameters() if n.startswith("pixel_decoder.")]
    params = [dict(head_o.named_parameters())[n] for n in names]
    loss = (mem_ref * dmem_ref).sum() + (MFr * dMF_ref).sum()
    gs = torch.autograd.grad(loss, f64 + params)
    report = []
    for l in range(3):
        _compare("features of level %d" % l, dfeats[l], gs[3 - l], report)
    _compare("features C2", dfeats[3], gs[0], report)
    for n, r in zip(names, gs[4:]):
        _compare(n, g[n], r, report)
    for n, r in head_grads.items():
        _compare(n, g[n], r, report)
    _print(report)
    assert set(g) == set(head.param_shapes()) - set(RR.UNREACHABLE)
    assert head.full_backward(grads, feats, pl=pl)[0][3] is None


def test_dropout_under_the_reference_masks():
    from pairnet_amd import BaselineHeadGrad
    from pairnet_amd.grad import FfnDropout
    head, sd, cls, _, pl, _ = _setup()
    drop = FfnDropout(0.1, seed=0x0123456789abcdef, subseq=1, step=7)
    tape = BaselineHeadGrad(head)
    plain = tape.forward_from_plan(pl)["rel"].clone()
    assert torch.equal(tape.forward_from_plan(pl, dropout=FfnDropout(0.0, seed=1))["rel"], plain)
    out = tape.forward_from_plan(pl, dropout=drop)
    assert float((out["rel"] - plain).abs().max()) > 1e-3           # dropout was not ignored
    grads = dict(_zero_seg_grads(pl), **_rel_grads(43))
    dmem, dMF, g = tape.backward(grads, counts=COUNTS)
    torch.cuda.synchronize()
    ref = _reference(tape, pl, sd, grads, drop=drop)
    for k, v in zip(("rel", "subject_scores", "object_scores"), ref[3]):
        err = float((out[k].cpu().double() - v).abs().max())
        print("dropped forward %s: %.2e" % (k, err))
        assert err < 1e-4
    report = []
    _compare_all(pl, dmem, dMF, g, ref, report, _all_names())
    _print(report)


def test_host_refusals():
    from pairnet_amd import BaselineHeadGrad, CrossHead2, CrossHeadBaseline
    head, sd, _, _, pl, feats = _setup()
    tape, _ = _tape()
    with pytest.raises(RuntimeError):
        BaselineHeadGrad(CrossHeadBaseline(**baseline_cfg()))           # not on the device
    grads = dict(_random_grads(9, 2, 100, 134, pl.hw2, COUNTS, seed=1), **_rel_grads(2))
    fresh = BaselineHeadGrad(head)
    with pytest.raises(RuntimeError):
        fresh.backward(grads, counts=COUNTS)                            # before forward_from_plan
    fresh.dt = tape.dt
    fresh.forward(tape.st["q"])                                         # the parent's heads only:
    with pytest.raises(RuntimeError):
        fresh.backward(grads, counts=COUNTS)                            # a tape without a relation stage
    keep = tape.flat_grad.clone()
    bad = [{k: v for k, v in grads.items() if k != "rel"},
           {k: v for k, v in grads.items() if k != "object_scores"},
           {k: v for k, v in grads.items() if k != "mask"},
           dict(grads, rel=grads["rel"][:, :, :56]), dict(grads, subject_scores=grads["rel"]),
           dict(grads, object_scores=grads["object_scores"][:1]),
           dict(grads, rel=grads["rel"].double()), dict(grads, subject_scores=grads["subject_scores"].cpu()),
           dict(grads, importance=grads["rel"]), dict(grads, cls=grads["cls"][:8])]
    for i, gb in enumerate(bad):
        with pytest.raises(ValueError):
            tape.backward(gb, counts=COUNTS)
            pytest.fail("grads %d were accepted" % i)
    algo = tape.attn_bwd_algo
    tape.attn_bwd_algo = "flash"
    try:
        with pytest.raises(ValueError):
            tape.backward(grads, counts=COUNTS)
    finally:
        tape.attn_bwd_algo = algo
    assert torch.equal(tape.flat_grad, keep)                            # refused before any launch
    head.return_all_layers = False
    try:
        head.forward(feats, [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)] * 2)
        with pytest.raises(RuntimeError):
            head.head_backward(grads)                                   # last-layer-only forward
    finally:
        head.return_all_layers = True
        head._last_plan = pl
