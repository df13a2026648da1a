"""GPU: whole training steps from odd images (tests/grad_shapes.py), checked for values.

`TailTrainer` at scope "all" (ResNet-50 stages 2-4 + pixel decoder + masked decoder + tail) on two
61 x 87 images -- the train pipeline's own odd batch tensor: C2 16 x 22 over 8 x 11, 4 x 6, 2 x 3,
ground-truth masks 30 x 43 -- against float64 autograd through the oracle ResNet, the oracle head
and the oracle's loss, tensor by tensor over the flat gradient buffer.  The float64 graph is fed what
is not differentiated exactly as the step had it: C2 (frozen stem and layer1), the attention-mask
bits of the nine masked layers, the selected pairs, and the step's own class / mask outputs for the
two Hungarian assignments (so the matches are the ones the HIP step made).  Tolerance as
tests/test_swin_full_gpu.py: 1e-4 of each tensor's largest float64 entry, or four times the
oracle's own fp32 run of the same graph where that is larger.

`BaselineTrainer` and `PSGTr2Trainer`: one step from 52 x 76 images against the manual composition
of the tapes (which tests/test_grad_shapes_gpu.py holds against float64 at that size), as
tests/test_baseline_train_gpu.py and tests/test_tri_train_gpu.py do at 64 x 96."""
import numpy as np
import pytest
import torch

import grad_shapes as GS
from helpers import head_cfg, oracle_head
from oracle.head import OracleCrossHead2
from oracle.losses import OracleCrossHead2Loss
from test_grad_gpu import TOL, _hip_head, _masked_layers, _tail

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _batch(s):
    g = torch.Generator().manual_seed(9)
    h, w = GS.gt_mask_size(s)
    img = torch.randn(s.B, 3, s.H, s.W, generator=g)
    gt_labels = [torch.tensor([3, 17, 90, 120, 3]), torch.tensor([5, 60, 7])]
    gt_masks = [torch.rand(5, h, w, generator=g) > 0.6, torch.rand(3, h, w, generator=g) > 0.5]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 3, 17], [1, 0, 56], [4, 2, 5], [0, 1, 9]]),
               torch.tensor([[0, 1, 2], [2, 1, 30]])]
    pts = [torch.rand(1, 12544, 2, generator=g) for _ in range(s.B)]
    return img, gt_rels, gt_labels, gt_masks, pts


def oracle_step(dtype, sd_head, sd_bb, c2, pl, tape, outs, batch):
    """The step's loss as a function of every trained parameter, by autograd in `dtype` on the CPU:
    oracle ResNet stages 2-4 from `c2`, oracle pixel decoder, the nine masked layers under `tape`'s
    mask bits, the tail on `pl`'s selected pairs (class logits detached, as the reference gathers
    them), `OracleCrossHead2Loss` with the detached outputs `outs` deciding the assignments ->
    ({flat-buffer name: gradient}, {loss term: value}, the differentiated logits).  (torch evaluates
    the oracle's `binary_cross_entropy_with_logits` in the fp32 of its 0 / 1 target even on float64
    logits: an elementwise term, 6e-8 of each entry of d loss_match / d importance, three decades
    below the tolerance; everything behind it is `dtype`.)"""
    from oracle.backbone import OracleResNet50
    bb = OracleResNet50()
    bb.load_state_dict(sd_bb)
    bb = bb.to(dtype).eval()
    head = OracleCrossHead2(**head_cfg()).eval()
    head.load_state_dict({k: v.detach().cpu() for k, v in sd_head.items()}, strict=True)
    head = head.to(dtype)
    for p in list(bb.parameters()) + list(head.parameters()):
        p.requires_grad_(True)
    x = c2.detach().cpu().to(dtype).contiguous()
    feats = [x]
    for i in (2, 3, 4):
        x = getattr(bb, "layer%d" % i)(x)
        feats.append(x)
    _, memories = head.pixel_decoder(feats)
    mem = torch.cat([m.flatten(2).transpose(1, 2) for m in memories], 1)
    q = _masked_layers(head, mem, pl, tape)
    o = _tail(head, q, pl.sub_pos.cpu(), pl.obj_pos.cpu(), cls_detached=True)
    cls, masks = outs
    fixed = lambda t: t.detach().cpu().float().clone()
    scores = dict(cls=fixed(cls["cls"]), sub=fixed(cls["sub"]), obj=fixed(cls["obj"]),
                  rel=o["rel"], importance=o["importance"])
    img, gt_rels, gt_labels, gt_masks, pts = batch
    losses = OracleCrossHead2Loss().loss(scores, dict(mask=fixed(masks["mask"])), gt_rels, gt_labels,
                                         gt_masks, point_coords=pts)
    (losses["loss_r_cls"] + losses["loss_match"]).backward()
    grads = {k: p.grad.double() for k, p in head.named_parameters() if p.grad is not None}
    grads.update({"backbone." + k: p.grad.double() for k, p in bb.named_parameters()
                  if p.grad is not None})
    return grads, {k: float(v.detach()) for k, v in losses.items()}, \
        {k: o[k].detach().double() for k in ("rel", "importance")}


def test_tail_trainer_full_scope_step_from_an_odd_image():
    from oracle.backbone import seeded_backbone_state
    from pairnet_amd import ResNet50Hip, TailTrainer
    s = GS.C
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    _, sd, _ = oracle_head(1234)
    head = _hip_head(sd)
    sd_bb = seeded_backbone_state(5)
    bb = ResNet50Hip()
    bb.load_state_dict(sd_bb)
    bb.to(DEV)
    batch = _batch(s)
    img, gt_rels, gt_labels, gt_masks, pts = batch
    img = img.to(DEV)
    metas = GS.metas(s)
    # what the step will see, kept before any parameter moves
    feats = [f.clone(memory_format=torch.preserve_format) for f in bb(img)]
    assert [tuple(f.shape[-2:]) for f in feats] == GS.pyramid(s.H, s.W)
    cls, masks = head.forward(feats, metas)
    outs = ({k: v.clone() for k, v in cls.items()}, {k: v.clone() for k, v in masks.items()})
    assert tuple(outs[1]["mask"].shape[-2:]) == GS.pyramid(s.H, s.W)[0]
    tr = TailTrainer(head, lr=1e-3, backbone=bb)
    out = tr.step(img, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
    torch.cuda.synchronize()
    pl = head._last_plan
    assert pl.B == s.B and list(pl.N) == GS.key_counts(s)
    flat = tr.flat_grad.cpu().double()
    ref, losses64, o64 = oracle_step(torch.float64, sd, sd_bb, feats[0], pl, tr.tape, outs, batch)
    ref32, _, _ = oracle_step(torch.float32, sd, sd_bb, feats[0], pl, tr.tape, outs, batch)
    # the differentiated outputs of the float64 graph are the step's own, and so are the losses
    for k in ("rel", "importance"):
        assert float((outs[0][k].cpu().double() - o64[k]).abs().max()) < 1e-4, k
    for k, v in losses64.items():
        print("%-14s HIP %.6f  float64 %.6f" % (k, float(out[k]), v))
        assert abs(float(out[k]) - v) < 1e-4 * max(1.0, abs(v)), k
    frozen = set(tr.layout) - set(tr.names)
    assert set(tr.names) <= set(ref), sorted(set(tr.names) - set(ref))[:5]
    assert sum(n.startswith("backbone.") for n in tr.names) == 42
    print("%-62s %10s %12s %12s" % ("tensor", "max |g|", "fp32 oracle", "HIP step"))
    bad, worst, slack = [], 0.0, 0.0
    for n, (o, shape, k) in tr.layout.items():
        got = flat[o:o + k].view(shape)
        if n in frozen:                                # the class path: no gradient in this graph
            assert float(got.abs().max()) == 0.0 and n not in ref, n
            continue
        assert tuple(ref[n].shape) == tuple(shape), n
        scale = float(ref[n].abs().max())
        assert scale > 0, n
        e32 = float((ref32[n] - ref[n]).abs().max()) / scale
        egpu = float((got - ref[n]).abs().max()) / scale
        worst = max(worst, egpu)
        slack += k * (max(TOL, 4.0 * e32) * scale) ** 2      # every entry off by the tensor's bound
        if not egpu <= TOL or e32 > TOL / 4:
            print("%-62s %10.3e %12.2e %12.2e" % (n, scale, e32, egpu))
        if not egpu <= max(TOL, 4.0 * e32):
            bad.append((n, egpu, e32))
    print("%d tensors, worst relative error %.2e" % (len(tr.names), worst))
    assert not bad, bad
    norm = float(torch.cat([ref[n].reshape(-1) for n in tr.names]).norm())
    # |norm(g) - norm(ref)| <= norm(g - ref) <= what the per-tensor bounds above allow together
    print("grad_norm: HIP %.6f, float64 %.6f (allowed %.2e)" % (float(out["grad_norm"]), norm,
                                                               np.sqrt(slack)))
    assert abs(float(out["grad_norm"]) - norm) <= np.sqrt(slack)


# ------------------------------------------------------------------------------ the other trainers
def test_baseline_trainer_step_from_52x76_images_is_the_manual_composition():
    import test_baseline_train_gpu as T
    s = T._first_step("image", (GS.A.H, GS.A.W))
    assert [tuple(f.shape[-2:]) for f in s["bb"](s["x"])] == GS.pyramid(GS.A.H, GS.A.W)
    T._check_twins(s, "image")


def test_psgtr2_trainer_step_from_52x76_images_is_the_manual_composition():
    import test_tri_train_gpu as T
    s = T._first_step("image", False, (GS.A.H, GS.A.W))
    assert [tuple(f.shape[-2:]) for f in s["bb"](s["x"])] == GS.pyramid(GS.A.H, GS.A.W)
    T._check_twins(s, "image", False)
