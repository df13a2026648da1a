"""GPU: `SegmenterHeadGrad` (pair-net_amd/seg_grad.py) -- the segmentation-loss gradients carried
through the class / mask heads and the nine masked decoder layers -- against float64 autograd: the
heads through the statement of tests/seg_grad_ref.py, the decoder through the reference-pinned
oracle's layers under the GPU's own attention-mask bits (as tests/test_grad_gpu.py does for
`HeadGrad`; the masks are `detach()`ed thresholds).  Tolerance: 1e-4 of each tensor's largest entry;
the taped forward reproduces the inference forward's stacks to 1e-4 absolute.  A seeded
`CrossHeadBaseline` at the 64 x 96 pyramid, `return_all_layers=True`, two images with 3 and 5
objects."""
import numpy as np
import pytest
import torch

import seg_grad_ref as R
from helpers import baseline_cfg, head_cfg, oracle_baseline_head, oracle_head
from oracle import seeded
from oracle.baseline_head import OracleCrossHeadBaseline
from test_grad_gpu import _compare, _compare_params, _print, _unpack_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 64, 96
COUNTS = [3, 5]
_S = {}


def _train_cfg():
    cc = lambda w: dict(type="ClassificationCost", weight=w)
    return dict(num_points=256, oversample_ratio=3.0, importance_sample_ratio=0.75,
                mask_assigner=dict(type="MaskHungarianAssigner", cls_cost=cc(2.0),
                                   mask_cost=dict(type="CrossEntropyLossCost", weight=5.0, use_sigmoid=True),
                                   dice_cost=dict(type="DiceCost", weight=5.0, pred_act=True, eps=1.0)),
                sampler=dict(type="MaskPseudoSampler"))


def _baseline(exact_mask_order=True):
    """(head, sd, cls, masks, pl) of one `return_all_layers=True` forward; cached per mask order."""
    if exact_mask_order not in _S:
        assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
        from pairnet_amd import CrossHeadBaseline
        _, sd, _ = oracle_baseline_head(1234)
        head = CrossHeadBaseline(**baseline_cfg(), train_cfg=_train_cfg())
        head.load_state_dict(sd)
        head.to(DEV)
        head.exact_mask_order = exact_mask_order
        head.return_all_layers = True
        feats = seeded.seeded_feats(99, 2, H, W)
        metas = [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)] * 2
        cls, masks = head.forward([f.to(DEV) for f in feats], metas)
        torch.cuda.synchronize()
        _S[exact_mask_order] = (head, sd, cls, masks, head._last_plan)
    return _S[exact_mask_order]


def _tape():
    if "tape" not in _S:
        from pairnet_amd import SegmenterHeadGrad
        head, _, _, _, pl = _baseline()
        tape = SegmenterHeadGrad(head)
        _S["tape"] = (tape, tape.forward_from_plan(pl, with_mask=True))
    return _S["tape"]


def _random_grads(L, B, Q, nc, hw, counts, seed, zero_layers=(), only_layer=None):
    """Random upstream gradients in the loss's compact form.  `zero_layers`: no class gradient and
    failed (-1) mask rows there; `only_layer`: that for every other layer."""
    g = torch.Generator().manual_seed(seed)
    g_cls = torch.randn(L, B, Q, nc, generator=g)
    rows = []
    for l in range(L):
        for b, n in enumerate(counts):
            rows.append(torch.randperm(Q, generator=g)[:n].sort()[0] + (l * B + b) * Q)
    rows = torch.cat(rows).long()
    g_mask = torch.randn(rows.numel(), hw[0], hw[1], generator=g)
    Ml = sum(counts)
    for l in range(L):
        if l in zero_layers or (only_layer is not None and l != only_layer):
            g_cls[l] = 0
            rows[l * Ml:(l + 1) * Ml] = -1
    return dict(cls=g_cls.to(DEV), mask=g_mask.to(DEV), mask_rows=rows.to(DEV))


def _oracle64(sd):
    head = OracleCrossHeadBaseline(**baseline_cfg()).eval()
    head.load_state_dict({k: v.detach().cpu() for k, v in sd.items()}, strict=True)
    return head.double()


def _reference(tape, pl, sd, grads, dtype=torch.float64):
    """Float64 autograd of the linear functional through the oracle's nine decoder layers (under the
    tape's mask bits) and the statement's heads -> (d mem, d MF, oracle head with .grad).  `dtype`:
    the same graph in fp32, for the oracle's own miss (tests/test_grad_gpu.py `_fp32_miss`)."""
    head_o = _oracle64(sd).to(dtype)
    B, Q = pl.B, tape.Q
    mem = pl.X.cpu().to(dtype).requires_grad_()
    MF = pl.MF.view(B, pl.HW2, 256).cpu().to(dtype).requires_grad_()
    keys, key_pos = [], []
    for l in range(3):
        h, w = pl.shapes[l]
        m = mem[:, pl.start[l]:pl.start[l] + pl.N[l]].transpose(0, 1)
        keys.append(m + head_o.level_embed.weight[l].view(1, 1, -1))
        pad = torch.zeros((B, h, w), dtype=torch.bool)
        key_pos.append(head_o.decoder_positional_encoding(pad).flatten(2).permute(2, 0, 1).to(dtype))
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
    R.functional(cls, mask, grads["cls"].cpu().to(dtype), grads["mask"].cpu().to(dtype),
                 grads["mask_rows"].cpu()).backward()
    return mem.grad, MF.grad, head_o


def _trunk_names(layers=range(9)):
    from pairnet_amd.grad import RelationTailGrad
    names = list(R.HEAD_PARAMS) + ["query_feat.weight", "query_embed.weight", "level_embed.weight"]
    for i in layers:
        names += RelationTailGrad._layer_names("transformer_decoder.layers.%d." % i)
    return names


@pytest.mark.parametrize("exact_mask_order", [True, False, "full"])
def test_taped_forward_equals_the_inference_forward(exact_mask_order):
    from pairnet_amd import SegmenterHeadGrad
    head, _, cls, masks, pl = _baseline(exact_mask_order)
    ref_cls, ref_mask = cls["cls"].clone(), masks["mask"].clone()
    if exact_mask_order is True:
        tape, out = _tape()
    else:
        out = SegmenterHeadGrad(head).forward_from_plan(pl, with_mask=True)
    torch.cuda.synchronize()
    assert out["cls"].shape == ref_cls.shape == (9, 2, 100, 134)
    assert out["mask"].shape == ref_mask.shape and out["me"].shape == (9 * 2 * 100, 256)
    e_cls = float((out["cls"] - ref_cls).abs().max())
    e_mask = float((out["mask"] - ref_mask).abs().max())
    print("taped forward (%s): cls %.2e, mask %.2e (max |mask| %.2f)"
          % (exact_mask_order, e_cls, e_mask, float(ref_mask.abs().max())))
    assert e_cls < 1e-4 and e_mask < 1e-4
    # the replay left the caller's outputs alone
    assert torch.equal(cls["cls"], ref_cls) and torch.equal(masks["mask"], ref_mask)


def test_heads_only_against_the_float64_statement():
    head, sd, _, _, pl = _baseline()
    tape, out = _tape()
    grads = _random_grads(9, 2, 100, 134, pl.hw2, COUNTS, seed=21, zero_layers=(2, 7))
    dmem, dMF, g = tape.backward(grads, counts=COUNTS)
    torch.cuda.synchronize()
    q_all = tape.st["q"].view(9, 2, 100, 256).cpu()
    MF = pl.MF.view(2, pl.HW2, 256).cpu()
    ref = R.vjp(q_all, MF, {k: v.cpu() for k, v in sd.items()}, grads["cls"].cpu(),
                grads["mask"].cpu(), grads["mask_rows"].cpu())
    report = []
    _compare("dq_all", tape.dq_all.view(9, 2, 100, 256), ref["q"], report)
    _compare("dMF", dMF, ref["MF"], report)
    for k in R.HEAD_PARAMS:
        _compare(k, g[k], ref[k], report)
    _print(report)
    for l in (2, 7):                                 # no upstream gradient: exact zeros
        assert float(tape.dq_all[l].abs().max()) == 0.0
    assert float(tape.dq_all[3].abs().max()) > 0


def test_end_to_end_from_the_heads_own_losses():
    head, sd, cls, masks, pl = _baseline()
    tape, out = _tape()
    gen = torch.Generator().manual_seed(8)
    gt_labels = [torch.randint(0, 133, (n,), generator=gen) for n in COUNTS]
    gt_masks = [(torch.rand(n, 32, 48, generator=gen) > 0.6).to(torch.uint8) for n in COUNTS]
    grads = {}
    losses = head.seg_losses(cls, masks, gt_labels, gt_masks, [dict()] * 2, grads=grads, seed=3)
    assert len(losses) == 27 and int(head.seg_status().cpu()) == 0
    assert head._seg_loss.last["counts"] == COUNTS and grads["mask"].shape[0] == 9 * sum(COUNTS)
    ends = []
    dmem, dMF, g = tape.backward(grads, on_ready=ends.append, counts=COUNTS)
    torch.cuda.synchronize()
    dmem_ref, dMF_ref, head_o = _reference(tape, pl, sd, grads)
    report = []
    _compare("memory tokens", dmem, dmem_ref, report)
    _compare("mask feature", dMF, dMF_ref, report)
    _compare_params(g, head_o, report, _trunk_names())
    _print(report)
    # flat layout: views of one buffer, on_ready ends monotone up to the whole buffer
    lo = tape.flat_grad.data_ptr()
    for n, (off, shape, numel) in tape.layout.items():
        assert g[n].data_ptr() == lo + 4 * off and tuple(g[n].shape) == shape and off % 64 == 0
    assert ends == sorted(ends) and ends[-1] == tape.flat_numel == tape.size_of(head)
    assert ends[0] == tape.group_end["heads"]
    # reuse: a second forward_from_plan + backward gives the same bits
    keep = (dmem.clone(), dMF.clone(), tape.flat_grad.clone())
    tape.forward_from_plan(pl)
    dmem2, dMF2, g2 = tape.backward(grads, counts=COUNTS)
    assert torch.equal(dmem2, keep[0]) and torch.equal(dMF2, keep[1])
    assert torch.equal(tape.flat_grad, keep[2])
    # the head's convenience returns the same triple
    dmem3, dMF3, g3 = head.seg_backward(grads)
    torch.cuda.synchronize()
    assert torch.equal(dmem3, keep[0]) and torch.equal(dMF3, keep[1])
    assert sorted(g3) == sorted(g) and all(torch.equal(g3[k], keep[2][o:o + n].view(s))
                                           for k, (o, s, n) in tape.layout.items())
    tape.forward_from_plan(pl, with_mask=True)       # (leave the shared tape as the others expect it)


def test_deep_supervision_reaches_only_the_layers_below():
    """Upstream gradients on layer 3 alone: layers 4-8 get exact zeros, layers 0-3 the reference's
    values -- which needs each layer's own head gradient added in on the way down."""
    head, sd, _, _, pl = _baseline()
    tape, out = _tape()
    grads = _random_grads(9, 2, 100, 134, pl.hw2, COUNTS, seed=34, only_layer=3)
    dmem, dMF, g = tape.backward(grads, counts=COUNTS)
    torch.cuda.synchronize()
    from pairnet_amd.grad import RelationTailGrad
    for i in range(4, 9):
        for n in RelationTailGrad._layer_names("transformer_decoder.layers.%d." % i):
            assert float(g[n].abs().max()) == 0.0, n
    dmem_ref, dMF_ref, head_o = _reference(tape, pl, sd, grads)
    report = []
    _compare("memory tokens", dmem, dmem_ref, report)
    _compare("mask feature", dMF, dMF_ref, report)
    _compare_params(g, head_o, report, _trunk_names(range(4)))
    _print(report)
    assert float(g["transformer_decoder.layers.0.ffns.0.layers.1.weight"].abs().max()) > 0


def test_refusals():
    from pairnet_amd import CrossHeadBaseline, SegmenterHeadGrad
    head, sd, _, _, pl = _baseline()
    with pytest.raises(RuntimeError):
        SegmenterHeadGrad(CrossHeadBaseline(**baseline_cfg()))         # not on the device
    fresh = SegmenterHeadGrad(head)
    grads = _random_grads(9, 2, 100, 134, pl.hw2, COUNTS, seed=1)
    with pytest.raises(RuntimeError):
        fresh.backward(grads, counts=COUNTS)                           # before forward_from_plan
    tape, _ = _tape()
    bad = [dict(grads, cls=grads["cls"][:8]), dict(grads, mask=grads["mask"][:, :-1]),
           dict(grads, mask_rows=grads["mask_rows"][:-1]), dict(grads, cls=grads["cls"].double()),
           dict(grads, mask=grads["mask"].cpu()), {k: v for k, v in grads.items() if k != "mask"}]
    for i, gb in enumerate(bad):
        with pytest.raises(ValueError):
            tape.backward(gb, counts=COUNTS)
            pytest.fail("grads %d were accepted" % i)
    for counts in ([3, 4], [8], None, [3, 5, 0]):
        with pytest.raises(ValueError):
            tape.backward(grads, counts=counts)
    head.return_all_layers = False
    try:
        one = head.forward([f.to(DEV) for f in seeded.seeded_feats(99, 2, H, W)],
                           [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)] * 2)
        with pytest.raises(RuntimeError):
            head.seg_backward(grads)                                   # last-layer-only forward
    finally:
        head.return_all_layers = True
        head._last_plan = pl


def test_the_same_tape_on_a_crosshead2_trunk():
    from pairnet_amd import CrossHead2, SegmenterHeadGrad
    _, sd, _ = oracle_head(1234)
    head = CrossHead2(**head_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    feats = seeded.seeded_feats(99, 1, H, W)
    head.forward([f.to(DEV) for f in feats], [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)])
    pl = head._last_plan
    tape = SegmenterHeadGrad(head)
    out = tape.forward_from_plan(pl)
    grads = _random_grads(9, 1, 100, 134, pl.hw2, [4], seed=55)
    dmem, dMF, g = tape.backward(grads)                # one image: counts follow from the shapes
    torch.cuda.synchronize()
    ref = R.vjp(tape.st["q"].view(9, 1, 100, 256).cpu(), pl.MF.view(1, pl.HW2, 256).cpu(),
                {k: v.cpu() for k, v in sd.items()}, grads["cls"].cpu(), grads["mask"].cpu(),
                grads["mask_rows"].cpu())
    report = []
    _compare("dq_all", tape.dq_all.view(9, 1, 100, 256), ref["q"], report)
    _compare("dMF", dMF, ref["MF"], report)
    for k in R.HEAD_PARAMS:
        _compare(k, g[k], ref[k], report)
    _print(report)
    assert bool(torch.isfinite(dmem).all()) and float(dmem.abs().max()) > 0
    assert float(g["query_feat.weight"].abs().max()) > 0
