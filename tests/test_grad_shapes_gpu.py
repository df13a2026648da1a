"""GPU: every training tape against float64 at the odd pyramids of tests/grad_shapes.py -- A
(52 x 76, two images: 13 x 19, 7 x 10, 4 x 5, 2 x 3) and B (72 x 100, three images: 18 x 25, 9 x 13,
5 x 7, 3 x 4) -- where ceil and floor part at every stride-2 step, no row count is a multiple of a
tile, the mask bits of a level end inside a word and the mask feature's rows are 19 and 25 wide.
The comparisons are the ones the tapes' own files make at 64 x 96 (their `_reference`, `_compare`,
`_compare_params`, `_trunk_names`), at the same tolerance: 1e-4 of each tensor's largest float64
entry (tests/test_grad_gpu.py `TOL`) -- or, per tensor, four times what the ORACLE's own fp32 run of
the same graph misses its float64 run by at that shape, where that is larger (`_compare`'s `e32`,
the rule of tests/test_swin_full_gpu.py): on these small maps one ReLU gate or one bilinear floor on
the other side of a jump moves a whole tensor by 1e-3 ... 3e-2, in torch's fp32 as on the GPU, and
the bound is measured from the oracle, never from the GPU.  Each such tensor is printed with both
figures.  tests/test_grad_shapes_refs.py proves the shapes and the references on the CPU;
`SegPixelDecoderGrad` has its odd pyramids in tests/test_fpn_grad_gpu.py."""
import pytest
import torch

import fpn_grad_ref as FR
import grad_shapes as GS
import rel_grad_ref as RR
import test_rel_grad_gpu as REL
import test_seg_grad_gpu as SEG
import test_tri_grad_gpu as TRI
from helpers import baseline_cfg, oracle_baseline_head, oracle_psgtr2_head, psgtr2_cfg
from oracle import seeded
from test_grad_gpu import (_check_backbone, _check_masked_decoder, _check_pixel_decoder, _compare,
                           _compare_params, _fp32_miss, _print)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAPE = pytest.mark.parametrize("shape", GS.TAPE_SHAPES, ids=[s.name for s in GS.TAPE_SHAPES])
_S = {}


def _levels(s):
    """(key counts C5, C4, C3; level sizes coarsest first; C2's size) of a shape."""
    pyr = GS.pyramid(s.H, s.W)
    return GS.key_counts(s), pyr[:0:-1], pyr[0]


def _check_plan(pl, s):
    N, sizes, c2 = _levels(s)
    assert pl.B == s.B and list(pl.N) == N and [tuple(x) for x in pl.shapes] == sizes
    assert tuple(pl.hw2) == c2 and pl.HW2 == c2[0] * c2[1]


# ------------------------------------------------------------------------------ grad.py's tapes
@TAPE
def test_pixel_decoder_backward(shape):
    got = _check_pixel_decoder(shape.H, shape.W, shape.B, fp32_rule=True)
    assert [g[-2:] for g in got] == _levels(shape)[1] and all(g[0] == shape.B for g in got)


@pytest.mark.parametrize("shape", GS.IMAGE_SHAPES, ids=[s.name for s in GS.IMAGE_SHAPES])
def test_backbone_backward_from_an_odd_image(shape):
    """C2 from `ResNet50Hip` on the image itself: at C both image sides are odd, so the stride-2
    3x3 convolutions and the projection shortcuts read odd inputs on both axes."""
    assert _check_backbone(shape.H, shape.W, shape.B, fp32_rule=True, tape_gates=True) == GS.pyramid(shape.H, shape.W)


@pytest.mark.parametrize("exact_mask_order", [True, False])
@TAPE
def test_masked_decoder_backward(shape, exact_mask_order):
    """The attention masks are resized to odd level sizes; 6 / 20 / 70 and 12 / 35 / 117 keys: the
    bit rows of every level end inside a word."""
    _check_plan(_check_masked_decoder(exact_mask_order, shape.H, shape.W, shape.B, fp32_rule=True,
                                      tape_gates=True), shape)


def _e32_of(ref64, ref32):
    """(d mem, d MF, oracle head) of a float64 and an fp32 run of one reference -> `_compare`'s e32."""
    return _fp32_miss({"memory tokens": ref64[0], "mask feature": ref64[1]},
                      {"memory tokens": ref32[0], "mask feature": ref32[1]}, ref64[2], ref32[2])


# ------------------------------------------------------------------------------ the sibling head
def _gt(s, seed=8):
    gen = torch.Generator().manual_seed(seed)
    h, w = GS.gt_mask_size(s)
    gt_labels = [torch.randint(0, 133, (n,), generator=gen) for n in s.counts]
    gt_masks = [(torch.rand(n, h, w, generator=gen) > 0.6).to(torch.uint8) for n in s.counts]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 0, 17], [1, 2, 55]]),
               torch.tensor([[0, 4, 2], [3, 1, 30], [4, 2, 9], [1, 0, 41]]),
               torch.tensor([[0, 1, 7], [1, 0, 23]])][:s.B]
    return gt_labels, gt_masks, gt_rels


def _baseline(s):
    """One `return_all_layers=True` forward of the seeded `CrossHeadBaseline` (the train_cfg of
    tests/test_rel_grad_gpu.py) per shape, and its `BaselineHeadGrad` tape."""
    key = ("baseline", s.name)
    if key not in _S:
        assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
        from pairnet_amd import BaselineHeadGrad, CrossHeadBaseline
        _, sd, _ = oracle_baseline_head(1234)
        cc = lambda w: dict(type="ClassificationCost", weight=w)
        tc = dict(SEG._train_cfg(), id_assigner=dict(type="OldIdMatcher", sub_id_cost=cc(1.0),
                                                     obj_id_cost=cc(1.0), r_cls_cost=cc(1.0)))
        head = CrossHeadBaseline(**baseline_cfg(), train_cfg=tc)
        head.load_state_dict(sd)
        head.to(DEV)
        head.exact_mask_order = True
        head.return_all_layers = True
        feats = [f.to(DEV) for f in seeded.seeded_feats(99, s.B, s.H, s.W)]
        cls, masks = head.forward(feats, GS.metas(s))
        torch.cuda.synchronize()
        pl = head._last_plan
        _check_plan(pl, s)
        tape = BaselineHeadGrad(head)
        out = tape.forward_from_plan(pl, with_mask=True)
        torch.cuda.synchronize()
        _S[key] = dict(head=head, sd=sd, cls=cls, masks=masks, pl=pl, feats=feats, tape=tape, out=out)
    return _S[key]


def _seg_grads(s):
    key = ("seg grads", s.name)
    if key not in _S:
        b = _baseline(s)
        gt_labels, gt_masks, _ = _gt(s)
        grads = {}
        losses = b["head"].seg_losses(b["cls"], b["masks"], gt_labels, gt_masks, [dict()] * s.B,
                                      grads=grads, seed=3)
        torch.cuda.synchronize()
        assert len(losses) == 27 and int(b["head"].seg_status().cpu()) == 0
        assert b["head"]._seg_loss.last["counts"] == list(s.counts)
        assert tuple(grads["mask"].shape) == (9 * sum(s.counts),) + _levels(s)[2]
        _S[key] = grads
    return _S[key]


def _full_grads(s):
    key = ("full grads", s.name)
    if key not in _S:
        b = _baseline(s)
        gt_labels, gt_masks, gt_rels = _gt(s)
        grads = {}
        losses = b["head"].full_losses(b["cls"], b["masks"], gt_rels, None, gt_labels, gt_masks,
                                       [dict()] * s.B, grads=grads, seed=3)
        torch.cuda.synchronize()
        assert len(losses) == 30 and sorted(grads) == sorted(
            ("cls", "mask", "mask_rows", "rel", "subject_scores", "object_scores"))
        assert b["head"]._seg_loss.last["counts"] == list(s.counts)
        _S[key] = grads
    return _S[key]


@TAPE
def test_taped_forwards_equal_the_inference_forward(shape):
    b = _baseline(shape)
    out, cls, masks = b["out"], b["cls"], b["masks"]
    c2 = _levels(shape)[2]
    assert out["cls"].shape == cls["cls"].shape == (9, shape.B, 100, 134)
    assert out["mask"].shape == masks["mask"].shape and tuple(out["mask"].shape[-2:]) == c2
    for k, ref in (("cls", cls["cls"]), ("mask", masks["mask"]), ("rel", cls["rel"]),
                   ("subject_scores", cls["subject_scores"]), ("object_scores", cls["object_scores"])):
        err = float((out[k] - ref).abs().max())
        print("taped %s at %s: %.2e (max |.| %.2f)" % (k, shape.name, err, float(ref.abs().max())))
        assert err < 1e-4, k


@pytest.mark.parametrize("min_keys", [None, 0], ids=["mha_bwd", "masked-keysplit"])
@TAPE
def test_segmenter_head_backward_from_its_own_losses(shape, min_keys):
    """`SegmenterHeadGrad` from `seg_losses` on ground-truth masks of (H // 2, W // 2): d memory,
    d mask feature, the trunk's and the heads' parameters; once more with all nine masked
    cross-attentions on `pn_mha_bwd_keysplit_masked_f32`."""
    from pairnet_amd import SegmenterHeadGrad, hip
    b = _baseline(shape)
    head, pl, sd = b["head"], b["pl"], b["sd"]
    grads = _seg_grads(shape)
    counts = list(shape.counts)
    tape = SegmenterHeadGrad(head)
    assert tape.masked_keysplit_min_keys is None
    tape.masked_keysplit_min_keys = min_keys
    tape.forward_from_plan(pl)
    calls = []
    real = hip.mha_bwd_keysplit
    hip.mha_bwd_keysplit = lambda *a, **kw: (calls.append(kw), real(*a, **kw))[1]
    try:
        dmem, dMF, g = tape.backward(grads, counts=counts)
    finally:
        hip.mha_bwd_keysplit = real
    torch.cuda.synchronize()
    assert len(calls) == (0 if min_keys is None else 9)
    dmem_ref, dMF_ref, head_o = SEG._reference(tape, pl, sd, grads)
    e32 = _e32_of((dmem_ref, dMF_ref, head_o), SEG._reference(tape, pl, sd, grads, torch.float32))
    report = []
    _compare("memory tokens", dmem, dmem_ref, report, e32)
    _compare("mask feature", dMF, dMF_ref, report, e32)
    _compare_params(g, head_o, report, SEG._trunk_names(), e32)
    _print(report)
    assert tuple(dMF.shape) == (shape.B, pl.HW2, 256) and float(dMF.abs().max()) > 0


def _names(head):
    from pairnet_amd import BaselineHeadGrad, SegmenterHeadGrad
    groups = BaselineHeadGrad.param_groups(head)
    branch = [n for _, names in groups[:len(groups) - len(SegmenterHeadGrad.param_groups(head))]
              for n in names]
    return branch + SEG._trunk_names()


@TAPE
def test_baseline_head_all_six_gradients_from_its_own_losses(shape):
    b = _baseline(shape)
    head, tape, pl, sd = b["head"], b["tape"], b["pl"], b["sd"]
    grads = _full_grads(shape)
    dmem, dMF, g = tape.backward(grads, counts=list(shape.counts))
    torch.cuda.synchronize()
    ref = REL._reference(tape, pl, sd, grads)
    report = []
    REL._compare_all(pl, dmem, dMF, g, ref, report, _names(head),
                     ref32=REL._reference(tape, pl, sd, grads, dtype=torch.float32))
    _print(report)
    assert set(g) == {k for k, p in ref[2].named_parameters() if p.grad is not None}
    assert set(g) == {k for k in head.param_shapes() if not k.startswith("pixel_decoder.")} - \
        set(RR.UNREACHABLE)


@TAPE
def test_baseline_head_through_the_pixel_decoder(shape):
    """`full_backward` against float64, as tests/test_rel_grad_gpu.py carries it on: the head's
    reference gradients through the oracle's pixel decoder, the FPN branch under the tape's gate."""
    b = _baseline(shape)
    head, tape, pl, sd, feats = b["head"], b["tape"], b["pl"], b["sd"], b["feats"]
    grads = _full_grads(shape)
    dfeats, g = head.full_backward(grads, feats, pl=pl, need_dc2=True)
    torch.cuda.synchronize()
    gate = (head._segpd_tape.t["fpn"]["Y"] > 0).permute(0, 3, 1, 2).cpu().double()

    def oracle(dtype):
        dmem_ref, dMF_ref, head_o, _ = REL._reference(tape, pl, sd, grads, dtype=dtype)
        out = {k: p.grad.clone() for k, p in head_o.named_parameters() if p.grad is not None}
        pd = head_o.pixel_decoder
        f = [x.cpu().to(dtype).requires_grad_() for x in feats]
        _, memories = pd(f)
        mem_ref = torch.cat([m.flatten(2).transpose(1, 2) for m in memories], 1)
        MFr, z = FR.branch(f[0], memories[2], FR.branch_params(pd), head.gn_groups, gate=gate)
        if dtype == torch.float64:
            assert FR.gate_mismatch(gate, z.detach()) <= FR.GATE_CAP
        MFr = MFr.flatten(2).transpose(1, 2)
        names = [n for n, _ in head_o.named_parameters() if n.startswith("pixel_decoder.")]
        params = [dict(head_o.named_parameters())[n] for n in names]
        gs = torch.autograd.grad((mem_ref * dmem_ref).sum() + (MFr * dMF_ref).sum(), f + params)
        out.update({"features of level %d" % l: gs[3 - l] for l in range(3)})
        out["features C2"] = gs[0]
        out.update(zip(names, gs[4:]))
        return out, names

    ref, names = oracle(torch.float64)
    e32 = _fp32_miss(ref, oracle(torch.float32)[0])
    report = []
    for l in range(3):
        _compare("features of level %d" % l, dfeats[l], ref["features of level %d" % l], report, e32)
    _compare("features C2", dfeats[3], ref["features C2"], report, e32)
    for n in ref:
        if not n.startswith("features"):
            _compare(n, g[n], ref[n], report, e32)
    _print(report)
    assert len(names) == 117 and set(g) == set(head.param_shapes()) - set(RR.UNREACHABLE)


# ------------------------------------------------------------------------------ PSGTrHead2
TRI_COUNTS = {"A": [3, 1], "B": [3, 1, 2]}


@TAPE
def test_psgtr2_head_backward(shape):
    """The clean case of tests/test_tri_grad_gpu.py: taped forward against the inference forward,
    then d memory, d mask feature and the 179 parameters against float64 autograd."""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import PSGTr2HeadGrad, PSGTrHead2
    _, sd, _ = oracle_psgtr2_head(1234)
    head = PSGTrHead2(**psgtr2_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    head.exact_mask_order = True
    feats = [f.to(DEV) for f in seeded.seeded_feats(99, shape.B, shape.H, shape.W)]
    cls, masks = head.forward(feats, GS.metas(shape))
    torch.cuda.synchronize()
    pl = head._last_plan
    _check_plan(pl, shape)
    keep = {k: v.clone() for k, v in list(cls.items()) + list(masks.items())}
    tape = PSGTr2HeadGrad(head)
    out = tape.forward_from_plan(pl, with_mask=True)
    torch.cuda.synchronize()
    for k in ("sub", "obj", "rel", "sub_seg", "obj_seg"):
        assert out[k].shape == keep[k].shape, k
        assert float((out[k] - keep[k]).abs().max()) < 1e-4, k
    counts = TRI_COUNTS[shape.name]
    grads = TRI._random_grads(pl, counts, seed=21)
    assert tuple(grads["sub_mask"].shape) == (sum(counts),) + _levels(shape)[2]
    dmem, dMF, g = tape.backward(grads, counts=counts)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tape.flat_grad).all()) and bool(torch.isfinite(dMF).all())
    flips = []
    dmem_ref, dMF_ref, head_o = TRI._reference(tape, pl, sd, grads, tape_gates=flips)
    print("FFN gates where the tape stands on the other side of 0 from float64:", flips)
    e32 = _e32_of((dmem_ref, dMF_ref, head_o),
                  TRI._reference(tape, pl, sd, grads, torch.float32, tape_gates=[]))
    names = [n for _, ns in PSGTr2HeadGrad.param_groups(head) for n in ns]
    assert len(names) == 179 and sorted(g) == sorted(names)
    report = []
    _compare("memory tokens", dmem, dmem_ref, report, e32)
    _compare("mask feature", dMF, dMF_ref, report, e32)
    _compare_params(g, head_o, report, names, e32)
    _print(report)
