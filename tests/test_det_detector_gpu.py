"""GPU: the plain Deformable-DETR detector (pair-net_amd/det_detector.py, det_head.py) at 128 x 160
(426 encoder tokens), B 2, one image padded (`img_shape` 112 x 160).

  * the four forward outputs against the oracle trunk (oracle/deformable_detr.py under
    oracle/bbox_head.py's branches: `trace["classes"]` / `trace["coords"]` are mmdet's per-layer
    logits and boxes) within the bounds tests/test_bbox_gpu.py applies to the same trunk: logits
    1e-3, boxes 1e-4, per-token logits 5e-5, per-token boxes 1e-5;
  * `CrossHeadBBox` on the same trunk weights: bitwise the same last-layer logits and boxes;
  * box results equal to the float64 statement of `_get_bboxes_single` on the GPU's own last-layer
    outputs (labels and grouping exact, boxes and scores under k_det_results' bound, L 3 + 4);
  * `val_det_losses`: the 21 finite keys; a state-dict round trip: bitwise the same outputs;
  * `detect(image)`: the od configs' pipeline (Pad 32) in front of `simple_test`;
  * the ResNeXt variant: build and one forward."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import det_loss_ref as R
from oracle import seeded
from test_grad_kernels_gpu import _within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 128, 160
METAS = [dict(batch_input_shape=(H, W), img_shape=(H, W, 3), scale_factor=np.array([1.0] * 4, np.float32)),
         dict(batch_input_shape=(H, W), img_shape=(112, 160, 3),
              scale_factor=np.array([1.25, 0.8, 1.25, 0.8], np.float32))]
TRUNK = ("transformer.", "cls_branches.", "reg_branches.")


def _err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _feats(seeds):
    per = [seeded.seeded_feats(int(s), 1, H, W)[1:] for s in seeds]
    return [torch.cat([p[l] for p in per], 0) for l in range(3)]


@pytest.fixture(scope="module")
def trunk(built_lib):
    """Oracle head + neck with seeded weights at 300 proposals (CrossHeadBBox's count), the HIP
    neck, the HIP detector head and CrossHeadBBox on the same weights, and both runs."""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import pairnet_amd as P
    from oracle.bbox_head import OracleCrossHeadBBox
    from oracle.deformable_detr import ChannelMapper
    cfg = {k: v for k, v in P.bbox_head_cfg().items() if k != "type"}
    ncfg = {k: v for k, v in P.channel_mapper_cfg().items() if k != "type"}
    ohead, oneck = OracleCrossHeadBBox(**cfg).eval(), ChannelMapper(**ncfg).eval()
    sd = seeded.seeded_state_dict(
        OrderedDict((k, tuple(v.shape)) for k, v in ohead.state_dict().items()), 12347)
    nsd = seeded.seeded_state_dict(
        OrderedDict((k, tuple(v.shape)) for k, v in oneck.state_dict().items()), 12348)
    ohead.load_state_dict(sd, strict=True)
    oneck.load_state_dict(nsd, strict=True)
    neck = P.ChannelMapper(**ncfg).to(DEV)
    neck.load_state_dict(nsd)
    dcfg = {k: v for k, v in P.det_head_cfg(num_query=300).items() if k != "type"}
    head = P.DeformableDETRHead(**dcfg, train_cfg=P.det_train_cfg()).to(DEV)
    head.load_state_dict(OrderedDict((k, v) for k, v in sd.items() if k.startswith(TRUNK)))
    box = P.CrossHeadBBox(**cfg).to(DEV)
    box.load_state_dict(sd)
    feats = _feats([100, 101])
    tr = {}
    with torch.no_grad():
        oc, _ = ohead(oneck(feats), METAS, trace=tr)
    outs = [t.clone() for t in head(neck([f.to(DEV) for f in feats]), METAS)]
    torch.cuda.synchronize()
    return dict(P=P, head=head, box=box, neck=neck, feats=feats, outs=outs, oracle=(oc, tr), sd=sd)


def test_forward_outputs_against_the_oracle_trunk(trunk):
    all_cls, all_box, enc_cls, enc_box = trunk["outs"]
    oc, tr = trunk["oracle"]
    assert tuple(all_cls.shape) == (6, 2, 300, 150) and tuple(all_box.shape) == (6, 2, 300, 4)
    assert tuple(enc_cls.shape) == (2, 426, 150) and tuple(enc_box.shape) == (2, 426, 4)
    assert trunk["head"]._last_plan.padded
    # The decoder's queries are the per-token proposals ranked by enc_cls[..., 0].  Two tokens whose
    # scores differ by less than the per-token logits' own bound may come out in the other order
    # (tests/test_bbox_gpu.py compares the proposal SETS for the same reason), and tokens without a
    # valid proposal tie exactly and are interchangeable.  The decoder is equivariant under a
    # permutation of its queries, so the rows are aligned by proposal token before they are compared:
    # the same valid tokens must be chosen, and every position where the order differs must be such
    # a near-tie.
    pl = trunk["head"]._last_plan
    got_idx, want_idx, valid = pl.top_idx.cpu(), tr["topk_proposals"], pl.valid.cpu().bool()
    score = oc["enc_cls_scores"][..., 0]
    perm = []
    for b in range(2):
        g, w_ = got_idx[b], want_idx[b]
        assert set(g[valid[b][g]].tolist()) == set(w_[valid[b][w_]].tolist())
        assert int((~valid[b][g]).sum()) == int((~valid[b][w_]).sum())
        pos = {int(t): i for i, t in enumerate(g.tolist()) if valid[b][t]}
        spare = [i for i, t in enumerate(g.tolist()) if not valid[b][t]]
        p_b = [pos[int(t)] if valid[b][t] else spare.pop(0) for t in w_.tolist()]
        moved = [j for j, i in enumerate(p_b) if i != j and valid[b][w_[j]]]
        print("image %d: %d valid proposals ranked in another order" % (b, len(moved)))
        for j in moved:
            assert abs(float(score[b, w_[j]]) - float(score[b, g[j]])) < 2 * 5e-5, (b, j)
        perm.append(torch.tensor(p_b))
    perm = torch.stack(perm).to(DEV)
    a_cls = torch.gather(all_cls, 2, perm[None, :, :, None].expand(6, 2, 300, 150))
    a_box = torch.gather(all_box, 2, perm[None, :, :, None].expand(6, 2, 300, 4))
    errs = dict(cls=_err(a_cls, tr["classes"]), box=_err(a_box, tr["coords"]),
                enc_cls=_err(enc_cls, oc["enc_cls_scores"]), enc_box=_err(enc_box, oc["enc_bbox_preds"]))
    print(errs)
    for i in range(6):
        print("layer %d  cls %.3e  box %.3e" % (i, _err(a_cls[i], tr["classes"][i]),
                                                 _err(a_box[i], tr["coords"][i])))
    assert errs["cls"] < 1e-3 and errs["box"] < 1e-4
    assert errs["enc_cls"] < 5e-5 and errs["enc_box"] < 1e-5
    # padded tokens of image 1 carry sigmoid(+inf) = 1
    inval = ~trunk["head"]._last_plan.valid.bool()
    assert int(inval[1].sum()) > int(inval[0].sum()) and bool((enc_box[inval] == 1.0).all())
    assert bool((all_box > 0).all()) and bool((all_box < 1).all())


def test_crossheadbbox_on_the_same_weights_is_bitwise_the_same_trunk(trunk):
    box, head, neck = trunk["box"], trunk["head"], trunk["neck"]
    box(neck([f.to(DEV) for f in trunk["feats"]]), METAS)
    torch.cuda.synchronize()
    pl = box._last_plan
    all_cls, all_box = trunk["outs"][0], trunk["outs"][1]
    assert torch.equal(pl.classes.view(2, 300, 150).view(torch.int32), all_cls[-1].view(torch.int32))
    assert torch.equal(pl.ref[-1].view(2, 300, 4).view(torch.int32), all_box[-1].view(torch.int32))
    assert torch.equal(pl.enc_cls.view(torch.int32), trunk["outs"][2].view(torch.int32))
    # the inference path (last layer only) gives the same last layer
    outs = head(neck([f.to(DEV) for f in trunk["feats"]]), METAS, all_layers=False)
    assert torch.equal(outs[0][-1], all_cls[-1]) and torch.equal(outs[1], all_box)


@pytest.mark.parametrize("rescale", [False, True])
def test_box_results_equal_the_statement_on_the_gpus_own_outputs(trunk, rescale):
    head, neck = trunk["head"], trunk["neck"]
    res = head.simple_test(neck([f.to(DEV) for f in trunk["feats"]]), METAS, rescale=rescale)
    all_cls, all_box = trunk["outs"][0].cpu(), trunk["outs"][1].cpu()
    assert len(res) == 2
    for b in range(2):
        m = METAS[b]
        ref, labels = R.get_bboxes_single(all_cls[-1, b], all_box[-1, b], m["img_shape"],
                                          m["scale_factor"], rescale, 100)
        want = R.bbox2result(ref.numpy(), labels.numpy(), 150)
        assert len(res[b]) == 150
        assert [len(r) for r in res[b]] == [len(w) for w in want] and sum(len(r) for r in res[b]) == 100
        got = torch.from_numpy(np.concatenate(res[b])).to(DEV)
        refc = torch.from_numpy(np.concatenate(want)).to(DEV)
        # the boxes behind the rows, in the grouped order, for the magnitude
        flat = np.lexsort((np.arange(300 * 150), -all_cls[-1, b].reshape(-1).double().numpy()))[:100]
        order = np.concatenate([np.nonzero(labels.numpy() == c)[0] for c in range(150)])
        bx = all_box[-1, b][torch.from_numpy(flat[order] // 150)].double()
        h, w = m["img_shape"][:2]
        sf = torch.tensor(m["scale_factor"], dtype=torch.float64) if rescale else torch.ones(4).double()
        wh = torch.tensor([w, h, w, h], dtype=torch.float64)
        mag = torch.cat([(bx[:, [0, 1, 0, 1]].abs() + 0.5 * bx[:, [2, 3, 2, 3]].abs()) * wh / sf,
                         refc[:, 4:].cpu()], -1).to(DEV)
        _within("simple_test image %d rescale %s" % (b, rescale), got, refc, mag, 3 + 4)
        assert bool((got[:, 0] >= 0).all()) and bool((got[:, 2] <= w / float(sf[2]) * (1 + 1e-6)).all())


def test_val_det_losses_and_state_dict_round_trip(trunk):
    P, head, neck = trunk["P"], trunk["head"], trunk["neck"]
    g = torch.Generator().manual_seed(9)
    gt_bboxes, gt_labels = [], []
    for m, G in zip(METAS, (4, 0)):
        h, w = m["img_shape"][:2]
        c, s = torch.rand(G, 2, generator=g) * 0.6 + 0.2, torch.rand(G, 2, generator=g) * 0.3 + 0.05
        gt_bboxes.append(torch.cat([c - s / 2, c + s / 2], -1) * torch.tensor([w, h, w, h], dtype=torch.float32))
        gt_labels.append(torch.randint(0, 150, (G,), generator=g))
    grads = {}
    losses = head.val_det_losses(neck([f.to(DEV) for f in trunk["feats"]]), METAS, gt_bboxes,
                                 gt_labels, grads=grads)
    assert list(losses) == R.keys(6) and len(losses) == 21
    assert all(v.dim() == 0 and v.is_cuda and bool(torch.isfinite(v)) for v in losses.values())
    assert all(float(losses[k]) > 0 for k in losses)
    assert tuple(grads["cls"].shape) == (6, 2, 300, 150) and tuple(grads["enc_bbox"].shape) == (2, 426, 4)
    assert bool((grads["bbox"][:, 1] == 0).all())                 # the image without ground truth
    # ---- a fresh head from the state dict: bitwise the same outputs ----
    dcfg = {k: v for k, v in P.det_head_cfg(num_query=300).items() if k != "type"}
    fresh = P.DeformableDETRHead(**dcfg).to(DEV)
    sd = head.state_dict()
    assert list(sd) == [k for k in trunk["sd"] if k.startswith(TRUNK)]
    fresh.load_state_dict(sd)
    outs = fresh(neck([f.to(DEV) for f in trunk["feats"]]), METAS)
    for a, b in zip(outs, trunk["outs"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(NotImplementedError):
        head.forward_train()


def test_detector_od_r101_end_to_end_and_resnext_forward(trunk):
    P = trunk["P"]
    from oracle.backbone import seeded_backbone_state
    import grouped_conv_ref as GR
    det = P.build_detector(P.od_r101_vg().model).to(DEV)
    det.backbone.load_state_dict(seeded_backbone_state(23, depth=101))
    det.neck.load_state_dict(trunk["neck"].state_dict())
    det.bbox_head.load_state_dict(OrderedDict(
        (k, v) for k, v in trunk["sd"].items() if k.startswith(TRUNK)))
    assert det.bbox_head.num_query == 100
    img = seeded.uniform(np.random.default_rng(24), (2, 3, H, W), -2.0, 2.0).to(DEV)
    metas = [dict(m) for m in METAS]
    res = det.simple_test(img, metas, rescale=True)
    assert len(res) == 2 and all(len(r) == 150 and sum(len(a) for a in r) == 100 for r in res)
    assert all(a.shape[1] == 5 and a.dtype == np.float32 for r in res for a in r)
    losses = det.val_det_losses(img, [dict(img_shape=m["img_shape"]) for m in METAS],
                                [torch.tensor([[10.0, 12.0, 90.0, 70.0]]), torch.zeros(0, 4)],
                                [torch.tensor([3]), torch.zeros(0, dtype=torch.int64)])
    assert len(losses) == 21 and all(bool(torch.isfinite(v)) for v in losses.values())
    # detect(image): the od configs' test pipeline (Pad to a multiple of 32) in front of simple_test
    pipe = det._pipeline_of_images()
    assert (pipe.img_scale, pipe.size_divisor) == ((1333, 800), 32)
    det.test_pipeline = P.TestPipeline(img_scale=(160, 128), size_divisor=32, device=DEV)
    image = np.random.default_rng(25).integers(0, 256, (100, 150, 3), dtype=np.uint8)
    got = det.detect(image, rescale=True)
    timg, tmetas = det.test_pipeline(image)
    assert tuple(timg.shape) == (1, 3, 128, 160) and tmetas[0]["img_shape"] == (107, 160, 3)
    want = det.simple_test(timg, tmetas, rescale=True)
    assert len(got) == 1 and len(got[0]) == 150 and sum(len(a) for a in got[0]) == 100
    assert all(np.array_equal(a, b) for a, b in zip(got[0], want[0]))
    boxes = np.concatenate(got[0])
    assert boxes[:, [0, 2]].max() <= 150 * (1 + 1e-6) and boxes[:, [1, 3]].max() <= 100 * (1 + 1e-6)
    # state-dict round trip at the detector level
    det2 = P.build_detector(P.od_r101_vg().model).to(DEV)
    det2.load_state_dict(det.state_dict())
    res2 = det2.simple_test(img, metas, rescale=True)
    assert all(np.array_equal(a, b) for r, s in zip(res, res2) for a, b in zip(r, s))
    del det, det2
    # ResNeXt-101 32x8d, 300 queries: build and one forward
    dx = P.build_detector(P.od_rnext101_vg().model).to(DEV)
    dx.backbone.load_state_dict(GR.seeded_state(71, 101))
    dx.neck.load_state_dict(trunk["neck"].state_dict())
    outs = dx.bbox_head(dx.extract_feat(img), metas)
    torch.cuda.synchronize()
    assert tuple(outs[0].shape) == (6, 2, 300, 150) and all(bool(torch.isfinite(o).all()) for o in outs)
