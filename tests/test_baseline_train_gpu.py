"""GPU: `BaselineTrainer` (pair-net_amd/baseline_train.py), one training iteration of the sibling
head, and its detector surface (`PSGTr.full_trainer` / `full_train_step`).  Setup as
`tests/test_rel_grad_gpu._setup`: the 64 x 96 pyramid, two images with 3 and 5 objects, the
`OldIdMatcher` train_cfg.  Two heads from one seeded state dict: a TWIN that is never trained (its
`full_losses` / `full_backward` are the statement) and the trained one; with a backbone, two
`ResNet50Hip` of one state dict likewise, and the step starts from the image."""
import numpy as np
import pytest
import torch

from helpers import baseline_cfg, oracle_baseline_head
from oracle import seeded
from test_seg_grad_gpu import COUNTS, _train_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 64, 96
SEED = 3
TOL_ATOMIC = 2 * 1e-4      # 2 x tests/test_grad_gpu.py's TOL (PixelDecoderGrad / BackboneGrad)
_S = {}


def _head(sd):
    from pairnet_amd import CrossHeadBaseline
    cc = lambda w: dict(type="ClassificationCost", weight=w)
    tc = dict(_train_cfg(), id_assigner=dict(type="OldIdMatcher", sub_id_cost=cc(1.0),
                                             obj_id_cost=cc(1.0), r_cls_cost=cc(1.0)))
    head = CrossHeadBaseline(**baseline_cfg(), train_cfg=tc)
    head.load_state_dict(sd)
    head.to(DEV)
    head.exact_mask_order = True
    return head


def _batch(H=H, W=W):
    gen = torch.Generator().manual_seed(8)
    gt_labels = [torch.randint(0, 133, (n,), generator=gen) for n in COUNTS]
    gt_masks = [(torch.rand(n, H // 2, W // 2, generator=gen) > 0.6).to(torch.uint8) for n in COUNTS]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 0, 17], [1, 2, 55]]),
               torch.tensor([[0, 4, 2], [3, 1, 30], [4, 2, 9], [1, 0, 41]])]
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)] * 2
    return metas, gt_rels, gt_labels, gt_masks


def _first_step(scope, hw=(H, W)):
    """One `step` of a fresh trainer beside the twin's statement; cached per scope ("feats": the
    four feature maps, backbone frozen; "image": ResNet stages 2-4 trained, from the image)."""
    key, (H, W) = (scope, hw), hw
    if key in _S:
        return _S[key]
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import BackboneGrad, BaselineTrainer, ResNet50Hip
    _, sd, _ = oracle_baseline_head(1234)
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
    twin.return_all_layers = True
    cls, masks = twin.forward(feats, metas)
    g = {}
    losses_t = twin.full_losses(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, grads=g,
                                seed=SEED, step=0)
    losses_t = {k: v.clone() for k, v in losses_t.items()}
    dfeats, grads_t = twin.full_backward(g, feats, pl=twin._last_plan)
    grads_t = {k: v.clone() for k, v in grads_t.items()}
    if bb_twin is not None:
        bt = BackboneGrad(bb_twin)
        bt.forward(feats[0])
        for k, v in bt.backward(dfeats[2], dfeats[1], dfeats[0]).items():
            grads_t["backbone." + k] = v.clone()
    # ---- the trained head ----
    before = {k: v.clone() for k, v in head.state_dict().items()}
    bb_before = {k: v.clone() for k, v in bb.state_dict().items()} if bb is not None else None
    tr = BaselineTrainer(head, backbone=bb, lr=1e-3, seed=SEED)
    p0 = tr.flat_p.clone()
    out = tr.step(x, metas, gt_rels, gt_labels, gt_masks)
    torch.cuda.synchronize()
    out = {k: v.clone() for k, v in out.items()}
    _S[key] = dict(tr=tr, head=head, bb=bb, sd=sd, x=x, p0=p0, out=out, losses_t=losses_t,
                     grads_t=grads_t, flat_grad=tr.flat_grad.clone(), flat_p1=tr.flat_p.clone(),
                     before=before, bb_before=bb_before, ends=list(tr.last_ready_ends))
    return _S[key]


@pytest.mark.parametrize("scope", ["feats", "image"])
def test_step_losses_and_gradients_are_the_twins(scope):
    _check_twins(_first_step(scope), scope)


def _check_twins(s, scope):
    from pairnet_amd import BaselineHeadGrad, SegPixelDecoderGrad
    tr, out = s["tr"], s["out"]
    assert set(out) == set(s["losses_t"]) | {"grad_norm", "assign_status"} and len(s["losses_t"]) == 30
    for k, v in s["losses_t"].items():
        assert torch.equal(out[k], v), k
    assert int(out["assign_status"]) == 0 and out["assign_status"].dtype == torch.int32
    assert tr.steps == 1
    exact = {n for _, names in BaselineHeadGrad.param_groups(tr.head) for n in names}
    exact |= {n for _, names in SegPixelDecoderGrad.BRANCH_GROUPS for n in names}
    assert set(tr.layout) == set(s["grads_t"])
    assert not any(n.startswith("relation_decoder.post_norm") for n in tr.layout)
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
    print("%s: %d exact tensors, the others within %.2e of their largest entry"
          % (scope, len(exact), worst))
    assert len(exact) > 250 and (scope == "feats") == (not any(n.startswith("backbone.") for n in tr.layout))
    # the tapes' on_ready ends: monotone over the one buffer, up to its end
    assert s["ends"] == sorted(s["ends"]) and s["ends"][-1] == tr.n == tr.flat_grad.numel()


@pytest.mark.parametrize("scope", ["feats", "image"])
def test_first_update_is_torchs_adamw_with_clip(scope):
    from pairnet_amd import BaselineTrainer
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
        hit = any(key in n for key in keys)
        is_norm = ".norms." in n or "post_norm" in n or ".gn." in n
        lm = 0.1 if hit else 1.0
        dm = 0.1 if hit else (0.0 if is_norm else 1.0)
        assert abs(float(tr.seg_lr[i]) - lm) < 1e-7 and abs(float(tr.seg_wd[i]) - dm) < 1e-7, n
        p = s["p0"][o:o + k].cpu().double().requires_grad_()
        opt = torch.optim.AdamW([p], lr=lr * lm, weight_decay=tr.wd * dm, betas=tr.betas, eps=tr.eps)
        p.grad = gflat[o:o + k] * coef
        opt.step()
        worst = max(worst, float((s["flat_p1"][o:o + k].cpu().double() - p.detach()).abs().max()))
    print("first AdamW update (%s): worst |difference| vs torch %.2e (lr %.0e)" % (scope, worst, lr))
    assert worst < 2e-2 * lr
    # one name of each kind
    mult = lambda n: (float(tr.seg_lr[list(tr.layout).index(n)]), float(tr.seg_wd[list(tr.layout).index(n)]))
    assert mult("transformer_decoder.layers.3.norms.1.weight") == pytest.approx((0.1, 0.1))    # key hit
    assert mult("pixel_decoder.input_convs.0.gn.weight") == pytest.approx((0.1, 0.1))           # key hit
    assert mult("relation_decoder.layers.2.norms.0.weight") == pytest.approx((1.0, 0.0))        # norm
    assert mult("rel_cls_embed.weight") == pytest.approx((1.0, 1.0))                            # plain
    assert mult("cls_embed.weight") == pytest.approx((1.0, 1.0))
    if scope == "image":
        assert mult("backbone.layer3.2.conv2.weight") == pytest.approx((0.1, 0.1))
    assert BaselineTrainer.multipliers("a.norms.0.bias", {"a.": 0.5}, {}, 0.0) == (0.5, 1.0)


@pytest.mark.parametrize("scope", ["feats", "image"])
def test_four_steps_write_back_and_a_fresh_model(scope):
    from pairnet_amd import CrossHeadBaseline, ResNet50Hip
    s = _first_step(scope)
    tr, head, bb, x = s["tr"], s["head"], s["bb"], s["x"]
    metas, gt_rels, gt_labels, gt_masks = _batch()
    hist = [sum(float(v) for k, v in s["out"].items() if "loss" in k)]
    while tr.steps < 4:
        out = tr.step(x, metas, gt_rels, gt_labels, gt_masks)
        assert int(out["assign_status"]) == 0
        assert all(np.isfinite(float(v)) for v in out.values())
        hist.append(sum(float(v) for k, v in out.items() if "loss" in k))
    print("summed loss per step (%s):" % scope, ["%.4f" % h for h in hist])
    tr.write_back()
    sd = head.state_dict()
    moved = {k for k in sd if not torch.equal(sd[k].cpu(), s["before"][k].cpu())}
    head_names = {n for n in tr.names if not n.startswith("backbone.")}
    assert moved == head_names, moved ^ head_names
    assert not any(k.startswith("relation_decoder.post_norm") for k in moved)
    assert "cls_embed.weight" in moved and "transformer_decoder.post_norm.weight" in moved
    feats = x
    if bb is not None:
        bsd = bb.state_dict()
        bmoved = {k for k in bsd if not torch.equal(bsd[k].cpu(), s["bb_before"][k].cpu())}
        assert bmoved == {n[len("backbone."):] for n in tr.names if n.startswith("backbone.")}
        assert len(bmoved) == 42 and not any(k.startswith(("conv1", "bn1", "layer1")) or ".bn" in k
                                             for k in bmoved)
        feats = [f.clone(memory_format=torch.preserve_format) for f in bb(x)]
        fresh_bb = ResNet50Hip()
        fresh_bb.load_state_dict(bsd)
        fresh_bb.to(DEV)
        for a, b_ in zip(fresh_bb(x), feats):
            assert torch.equal(a, b_)
    head.return_all_layers = True
    cls, masks = head.forward(feats, metas)
    want = {k: cls[k].clone() for k in ("cls", "rel", "subject_scores", "object_scores")}
    want["mask"] = masks["mask"].clone()
    fresh = CrossHeadBaseline(**baseline_cfg())
    fresh.load_state_dict(sd)
    fresh.to(DEV)
    fresh.exact_mask_order = True
    fresh.return_all_layers = True
    cls2, masks2 = fresh.forward(feats, metas)
    torch.cuda.synchronize()
    for k in ("cls", "rel", "subject_scores", "object_scores"):
        assert torch.equal(cls2[k], want[k]), k
    assert torch.equal(masks2["mask"], want["mask"])


def test_a_refused_assignment_moves_no_parameter():
    from pairnet_amd import hip
    s = _first_step("feats")
    tr, x = s["tr"], s["x"]
    metas, gt_rels, gt_labels, gt_masks = _batch()
    keep = [t.clone() for t in (tr.flat_p, tr.flat_m, tr.flat_v)]
    steps = tr.steps
    # (a device tensor is range-checked on the device: object 7 of an image with 5 objects)
    bad = [gt_rels[0].to(DEV), torch.tensor([[0, 7, 2], [3, 1, 30]], device=DEV)]
    out = tr.step(x, metas, bad, gt_labels, gt_masks)
    torch.cuda.synchronize()
    assert int(out["assign_status"]) & hip.REL_STATUS_RANGE
    for a, b in zip((tr.flat_p, tr.flat_m, tr.flat_v), keep):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert tr.steps == steps + 1
    out = tr.step(x, metas, gt_rels, gt_labels, gt_masks)           # the next clean batch moves them
    torch.cuda.synchronize()
    assert int(out["assign_status"]) == 0 and not torch.equal(tr.flat_p, keep[0])


def test_detector_surface():
    from pairnet_amd import (BaselineTrainer, SwinTransformerHip, baseline_r50, build_detector,
                             pairnet_r50, swin_backbone_cfg)
    with pytest.raises(NotImplementedError):
        build_detector(pairnet_r50()).full_trainer()                 # a CrossHead2 detector
    _, sd, _ = oracle_baseline_head(1234)
    det = build_detector(baseline_r50())
    det.bbox_head.load_state_dict(sd)
    det.to(DEV)
    with pytest.raises(NotImplementedError):
        det.trainer()                                                # still refuses the sibling head
    with pytest.raises(NotImplementedError):
        det.train_step(None, None)
    g = torch.Generator().manual_seed(9)
    img = torch.randn(2, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4, batch_input_shape=(H, W))] * 2
    _, gt_rels, gt_labels, _ = _batch()
    gt_masks = [(torch.rand(n, H, W, generator=g) > 0.6).numpy() for n in COUNTS]
    # from the image (the default for a ResNet backbone), forward_train's argument order
    out = det.full_train_step(img, metas, gt_rels, None, gt_labels, gt_masks)
    tr = det._full_trainer
    assert isinstance(tr, BaselineTrainer) and tr.backbone is det.backbone and tr.steps == 1
    assert len(out) == 32 and int(out["assign_status"]) == 0 and float(out["grad_norm"]) > 0
    # mmdet's form
    rec = det.full_train_step(dict(img=img, img_metas=metas, gt_rels=gt_rels, gt_bboxes=None,
                                   gt_labels=gt_labels, gt_masks=gt_masks), None)
    assert set(rec) == {"loss", "log_vars", "num_samples"} and rec["num_samples"] == 2
    terms = [v for k, v in rec["log_vars"].items() if "loss" in k and k != "loss"]
    assert len(terms) == 30 and abs(float(rec["loss"]) - sum(terms)) < 1e-3 * sum(terms)
    assert tr.steps == 2 and det._full_trainer is tr
    assert tr.set_epoch(0) == tr.base_lr and tr.set_epoch(40) == pytest.approx(0.1 * tr.base_lr)
    tr.set_epoch(0)
    # features only: the backbone stays
    bb0 = {k: v.clone() for k, v in det.backbone.state_dict().items()}
    tr2 = det.full_trainer(train_backbone=False, lr=1e-3)
    assert tr2.backbone is None and not any(n.startswith("backbone.") for n in tr2.names)
    out = det.full_train_step(img, metas, gt_rels, None, gt_labels, gt_masks)
    assert tr2.steps == 1 and np.isfinite(float(out["loss_cls"]))
    tr2.write_back()
    assert all(torch.equal(v.cpu(), bb0[k].cpu()) for k, v in det.backbone.state_dict().items())
    assert len(det.simple_test(img[:1], metas[:1])) == 1             # inference on the trained weights
    # refusals: a re-packed head, a Swin backbone
    det.bbox_head.load_state_dict(det.bbox_head.state_dict())
    det.simple_test(img[:1], metas[:1])
    with pytest.raises(RuntimeError, match="re-packed"):
        tr2.step(list(det.extract_feat(img)), metas, gt_rels, gt_labels,
                 det._prepare_gt_masks(img, gt_masks))
    swin = SwinTransformerHip(**{k: v for k, v in swin_backbone_cfg("T").items() if k != "type"})
    with pytest.raises(NotImplementedError):
        BaselineTrainer(det.bbox_head, backbone=swin)
    from pairnet_amd import CrossHead2
    from helpers import head_cfg
    with pytest.raises(NotImplementedError):
        BaselineTrainer(CrossHead2(**head_cfg()))
