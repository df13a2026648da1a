"""GPU: `PSGTr2Trainer` (pair-net_amd/psgtr2_train.py), one training iteration of `PSGTrHead2`, and
its detector surface (`PSGTr.triplet_trainer` / `triplet_train_step`).  Setup as
tests/test_baseline_train_gpu.py: the 64 x 96 pyramid, two images with 3 and 5 objects.  Two heads
from one seeded state dict: a TWIN that is never trained (its `triplet_losses` / `triplet_backward`
are the statement) and the trained one; with a backbone, two `ResNet50Hip` of one state dict
likewise, and the step starts from the image."""
import numpy as np
import pytest
import torch

import tri_grad_ref as R
from helpers import oracle_psgtr2_head, psgtr2_cfg
from oracle import seeded
from test_baseline_train_gpu import TOL_ATOMIC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 64, 96
SEED = 3
OBJECTS = [3, 5]
_S = {}


def _head(sd):
    from pairnet_amd import PSGTrHead2
    head = PSGTrHead2(**psgtr2_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    head.exact_mask_order = True
    return head


def _batch(H=H, W=W):
    gen = torch.Generator().manual_seed(8)
    gt_labels = [torch.randint(0, 133, (n,), generator=gen) for n in OBJECTS]
    gt_masks = [(torch.rand(n, H // 2, W // 2, generator=gen) > 0.6).to(torch.uint8) for n in OBJECTS]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 0, 17], [1, 2, 55]]),
               torch.tensor([[0, 4, 2], [3, 1, 30], [4, 2, 9], [1, 0, 41]])]
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)] * 2
    return metas, gt_rels, gt_labels, gt_masks


def _first_step(scope, deterministic=False, hw=(H, W)):
    """One `step` of a fresh trainer beside the twin's statement; cached per scope ("feats": the
    four feature maps, backbone frozen; "image": ResNet stages 2-4 trained, from the image)."""
    key = (scope, deterministic, hw)
    H, W = hw
    if key in _S:
        return _S[key]
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import BackboneGrad, PSGTr2Trainer, ResNet50Hip
    _, sd, _ = oracle_psgtr2_head(1234)
    twin, head = _head(sd), _head(sd)
    metas, gt_rels, gt_labels, gt_masks = _batch(H, W)
    bb = bb_twin = None
    if scope == "image":
        bb = ResNet50Hip().to(DEV)
        bb_twin = ResNet50Hip()
        bb_twin.load_state_dict(bb.state_dict())
        bb_twin.to(DEV)
        x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(5)).to(DEV)
        feats = [f.clone(memory_format=torch.preserve_format) for f in bb_twin(x)]
    else:
        x = feats = [f.to(DEV) for f in seeded.seeded_feats(99, 2, H, W)]
    # ---- the twin's statement ----
    cls, masks = twin.forward(feats, metas)
    g = {}
    losses_t = twin.triplet_losses(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, grads=g,
                                   seed=SEED, step=0)
    losses_t = {k: v.clone() for k, v in losses_t.items()}
    dfeats, grads_t = twin.triplet_backward(g, feats, pl=twin._last_plan,
                                            deterministic=deterministic)
    grads_t = {k: v.clone() for k, v in grads_t.items()}
    if bb_twin is not None:
        bt = BackboneGrad(bb_twin)
        bt.forward(feats[0])
        for k, v in bt.backward(dfeats[2], dfeats[1], dfeats[0]).items():
            grads_t["backbone." + k] = v.clone()
    # ---- the trained head ----
    before = {k: v.clone() for k, v in head.state_dict().items()}
    bb_before = {k: v.clone() for k, v in bb.state_dict().items()} if bb is not None else None
    tr = PSGTr2Trainer(head, backbone=bb, lr=1e-3, seed=SEED, deterministic=deterministic)
    p0 = tr.flat_p.clone()
    out = tr.step(x, metas, gt_rels, gt_labels, gt_masks)
    torch.cuda.synchronize()
    out = {k: v.clone() for k, v in out.items()}
    _S[key] = dict(tr=tr, head=head, bb=bb, sd=sd, x=x, p0=p0, out=out, losses_t=losses_t,
                   grads_t=grads_t, flat_grad=tr.flat_grad.clone(), flat_p1=tr.flat_p.clone(),
                   before=before, bb_before=bb_before, ends=list(tr.last_ready_ends))
    return _S[key]


@pytest.mark.parametrize("scope,deterministic", [("feats", False), ("image", False), ("feats", True)])
def test_step_losses_and_gradients_are_the_twins(scope, deterministic):
    _check_twins(_first_step(scope, deterministic), scope, deterministic)


def _check_twins(s, scope, deterministic):
    from pairnet_amd import PSGTr2HeadGrad, SegPixelDecoderGrad
    tr, out = s["tr"], s["out"]
    assert set(out) == set(s["losses_t"]) | {"grad_norm", "assign_status"} and len(s["losses_t"]) == 7
    for k, v in s["losses_t"].items():
        assert torch.equal(out[k], v) and np.isfinite(float(v)), k
    assert int(out["assign_status"]) == 0 and out["assign_status"].dtype == torch.int32
    assert tr.steps == 1
    exact = {n for _, names in PSGTr2HeadGrad.param_groups(tr.head) for n in names}
    exact |= {n for _, names in SegPixelDecoderGrad.BRANCH_GROUPS for n in names}
    if deterministic:
        exact = set(tr.layout)
    assert set(tr.layout) == set(s["grads_t"])
    assert not any(n.startswith(("mask_embed.", "sub_mask_embed.")) for n in tr.layout)
    worst = 0.0
    for n, (o, shape, k) in tr.layout.items():
        got, ref = s["flat_grad"][o:o + k].view(shape), s["grads_t"][n]
        if n in exact:
            assert torch.equal(got, ref), n
        else:       # behind pn_msda_bwd_f32's float atomics: not reproducible bit for bit
            scale = float(ref.abs().max())
            err = float((got - ref).abs().max())
            worst = max(worst, err / scale if scale else 0.0)
            assert err <= TOL_ATOMIC * scale, (n, err, scale)
    print("%s (deterministic %s): %d exact tensors, the others within %.2e of their largest entry"
          % (scope, deterministic, len(exact), worst))
    assert len(exact) >= 179 + 8
    assert (scope == "feats") == (not any(n.startswith("backbone.") for n in tr.layout))
    assert float(s["flat_grad"].abs().max()) > 0
    assert s["ends"] == sorted(s["ends"]) and s["ends"][-1] == tr.n == tr.flat_grad.numel()


@pytest.mark.parametrize("scope", ["feats", "image"])
def test_first_update_is_torchs_adamw_with_clip(scope):
    s = _first_step(scope)
    tr, lr = s["tr"], 1e-3
    gflat = s["flat_grad"].cpu().double()
    norm = float(gflat.norm())
    assert abs(float(s["out"]["grad_norm"]) - norm) < 1e-4 * norm and norm > 0
    coef = min(1.0, tr.max_norm / (norm + 1e-6))
    keys = ("backbone", "transformer_decoder", "pixel_decoder", "decoder_input_projs")
    worst = 0.0
    for i, n in enumerate(tr.layout):
        o, shape, k = tr.layout[n]
        lm = 0.1 if any(key in n for key in keys) else 1.0          # decay_mult 1.0, no norm rule
        assert abs(float(tr.seg_lr[i]) - lm) < 1e-7 and abs(float(tr.seg_wd[i]) - 1.0) < 1e-7, n
        p = s["p0"][o:o + k].cpu().double().requires_grad_()
        opt = torch.optim.AdamW([p], lr=lr * lm, weight_decay=tr.wd, betas=tr.betas, eps=tr.eps)
        p.grad = gflat[o:o + k] * coef
        opt.step()
        worst = max(worst, float((s["flat_p1"][o:o + k].cpu().double() - p.detach()).abs().max()))
    print("first AdamW update (%s): worst |difference| vs torch %.2e (lr %.0e)" % (scope, worst, lr))
    assert worst < 2e-2 * lr
    mult = lambda n: (float(tr.seg_lr[list(tr.layout).index(n)]), float(tr.seg_wd[list(tr.layout).index(n)]))
    assert mult("transformer_decoder.layers.3.norms.1.weight") == pytest.approx((0.1, 1.0))
    assert mult("sub_cls_embed.weight") == pytest.approx((1.0, 1.0))
    assert mult("obj_mask_embed.0.bias") == pytest.approx((1.0, 1.0))
    if scope == "image":
        assert mult("backbone.layer3.2.conv2.weight") == pytest.approx((0.1, 1.0))


@pytest.mark.parametrize("scope", ["feats", "image"])
def test_write_back_and_a_fresh_model(scope):
    from pairnet_amd import PSGTrHead2, ResNet50Hip
    s = _first_step(scope)
    tr, head, bb, x = s["tr"], s["head"], s["bb"], s["x"]
    metas, gt_rels, gt_labels, gt_masks = _batch()
    if tr.steps < 2:
        out = tr.step(x, metas, gt_rels, gt_labels, gt_masks)
        assert int(out["assign_status"]) == 0 and all(np.isfinite(float(v)) for v in out.values())
    tr.write_back()
    sd = head.state_dict()
    moved = {k for k in sd if not torch.equal(sd[k].cpu(), s["before"][k].cpu())}
    head_names = {n for n in tr.names if not n.startswith("backbone.")}
    assert moved == head_names, moved ^ head_names
    for k in R.UNREACHED:                   # neither decayed nor moved: bit for bit
        assert torch.equal(sd[k].cpu().view(torch.int32), s["before"][k].cpu().view(torch.int32)), k
        assert torch.equal(head.w[k].view(torch.int32), s["before"][k].to(DEV).view(torch.int32)), k
    assert "sub_cls_embed.weight" in moved and "query_feat.weight" in moved
    feats = x
    if bb is not None:
        bsd = bb.state_dict()
        bmoved = {k for k in bsd if not torch.equal(bsd[k].cpu(), s["bb_before"][k].cpu())}
        assert bmoved == {n[len("backbone."):] for n in tr.names if n.startswith("backbone.")}
        assert len(bmoved) == 42
        feats = [f.clone(memory_format=torch.preserve_format) for f in bb(x)]
        fresh_bb = ResNet50Hip()
        fresh_bb.load_state_dict(bsd)
        fresh_bb.to(DEV)
        for a, b_ in zip(fresh_bb(x), feats):
            assert torch.equal(a, b_)
    cls, masks = head.forward(feats, metas)
    want = {k: v.clone() for k, v in list(cls.items()) + list(masks.items())}
    fresh = PSGTrHead2(**psgtr2_cfg())
    fresh.load_state_dict(sd)
    fresh.to(DEV)
    fresh.exact_mask_order = True
    cls2, masks2 = fresh.forward(feats, metas)
    torch.cuda.synchronize()
    for k, v in list(cls2.items()) + list(masks2.items()):
        assert torch.equal(v, want[k]), k            # every derived pack was refreshed


def test_a_refused_assignment_moves_no_parameter():
    s = _first_step("feats")
    tr, x = s["tr"], s["x"]
    metas, gt_rels, gt_labels, gt_masks = _batch()
    keep = [t.clone() for t in (tr.flat_p, tr.flat_m, tr.flat_v)]
    steps = tr.steps
    # (a device tensor is range-checked on the device: object 7 of an image with 5 objects)
    bad = [gt_rels[0].to(DEV), torch.tensor([[0, 7, 2], [3, 1, 30]], device=DEV)]
    out = tr.step(x, metas, bad, gt_labels, gt_masks)
    torch.cuda.synchronize()
    assert int(out["assign_status"]) != 0
    for a, b in zip((tr.flat_p, tr.flat_m, tr.flat_v), keep):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert tr.steps == steps + 1
    out = tr.step(x, metas, gt_rels, gt_labels, gt_masks)           # the next clean batch moves them
    torch.cuda.synchronize()
    assert int(out["assign_status"]) == 0 and not torch.equal(tr.flat_p, keep[0])


def test_detector_surface():
    from pairnet_amd import (PSGTr2Trainer, SwinTransformerHip, build_detector, pairnet_r50,
                             psgtr2_r50, swin_backbone_cfg)
    with pytest.raises(NotImplementedError):
        build_detector(pairnet_r50()).triplet_trainer()              # a CrossHead2 detector
    _, sd, _ = oracle_psgtr2_head(1234)
    det = build_detector(psgtr2_r50())
    det.bbox_head.load_state_dict(sd)
    det.to(DEV)
    with pytest.raises(NotImplementedError):
        det.trainer()                                                # still refuses this head
    with pytest.raises(NotImplementedError):
        det.train_step(None, None)
    g = torch.Generator().manual_seed(9)
    img = torch.randn(2, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4, batch_input_shape=(H, W))] * 2
    _, gt_rels, gt_labels, _ = _batch()
    gt_masks = [(torch.rand(n, H, W, generator=g) > 0.6).numpy() for n in OBJECTS]
    # the statement: a trainer of its own on a second detector of the same weights
    det2 = build_detector(psgtr2_r50())
    det2.bbox_head.load_state_dict(sd)
    det2.backbone.load_state_dict(det.backbone.state_dict())
    det2.to(DEV)
    tr2 = det2.triplet_trainer()
    want = tr2.step(img, metas, gt_rels, gt_labels, det2._prepare_gt_masks(img, gt_masks))
    want = {k: v.clone() for k, v in want.items()}
    # forward_train's argument order, from the image (the default for a ResNet backbone)
    out = det.triplet_train_step(img, metas, gt_rels, None, gt_labels, gt_masks)
    tr = det._triplet_trainer
    assert isinstance(tr, PSGTr2Trainer) and tr.backbone is det.backbone and tr.steps == 1
    assert len(out) == 9 and int(out["assign_status"]) == 0 and float(out["grad_norm"]) > 0
    for k in want:
        if "loss" in k:
            assert torch.equal(out[k], want[k]), k
    # mmdet's form: the second step of both
    want2 = tr2.step(img, metas, gt_rels, gt_labels, det2._prepare_gt_masks(img, gt_masks))
    rec = det.triplet_train_step(dict(img=img, img_metas=metas, gt_rels=gt_rels, gt_bboxes=None,
                                      gt_labels=gt_labels, gt_masks=gt_masks), None)
    assert set(rec) == {"loss", "log_vars", "num_samples"} and rec["num_samples"] == 2
    terms = {k: v for k, v in rec["log_vars"].items() if "loss" in k and k != "loss"}
    assert len(terms) == 7 and abs(float(rec["loss"]) - sum(terms.values())) < 1e-3 * sum(terms.values())
    for k, v in terms.items():          # (float atomics in the first step's pixel-decoder gradients)
        assert abs(v - float(want2[k])) <= 1e-3 * abs(float(want2[k])), k
    assert tr.steps == 2 and det._triplet_trainer is tr
    assert tr.set_epoch(0) == tr.base_lr and tr.set_epoch(40) == pytest.approx(0.1 * tr.base_lr)
    swin = SwinTransformerHip(**{k: v for k, v in swin_backbone_cfg("T").items() if k != "type"})
    with pytest.raises(NotImplementedError):
        PSGTr2Trainer(det.bbox_head, backbone=swin)
