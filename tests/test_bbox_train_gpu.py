"""GPU: the box head's tape (`BBoxTailGrad`, pair-net_amd/grad.py) and training step
(`BBoxTrainer`, pair-net_amd/bbox_train.py) on the full-size head of `bbox_head_cfg()` (300
proposals, 100 kept), B = 2.

The features are those of a 128 x 160 image (levels 16x20, 8x10, 4x5, 2x3: 426 encoder tokens).  A
64 x 80 image has 108 tokens, fewer than the 300 proposals the full-size head selects, and the head
refuses it; 128 x 160 is the smallest image of that aspect the head accepts.  The weights are the
project's seeded state dict (oracle/seeded.py), the ones tests/test_bbox_gpu.py checks this head's
inference with.  (With `init_weights`' N(0, 1) embeddings instead, the first run measured 5.6e-5
relative on `relation_decoder.layers.4.attentions.0.attn.in_proj_weight`, max |g| 11.7.)

  * the tape's forward reproduces `head.forward`'s rel / importance / sub / obj to 1e-4 absolute,
    the tolerance tests/test_grad_gpu.py applies to `RelationTailGrad`;
  * every gradient equals float64 autograd through `OracleCrossHeadBBox`'s own modules from the
    same kept queries and the same pair list, to 1e-5 of each tensor's largest entry (README
    "Training");
  * the first AdamW update is bounded against torch's AdamW + clip on the tape's own gradients, as
    tests/test_swin_full_gpu.py bounds it (2e-2 lr);
  * parameters outside the layout do not move; after a step, inference through the trained head
    equals bit for bit a fresh head loaded from `write_back()`'s state dict; a planted NaN with
    `device_targets=True` changes no bit of the parameters, m or v; two runs give equal bits.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bbox_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, B = 128, 160, 2
SHAPES = [(16, 20), (8, 10), (4, 5), (2, 3)]


def _cfg():
    import pairnet_amd as P
    return {k: v for k, v in P.bbox_head_cfg().items() if k != "type"}


def _head(sd=None, seed=3):
    """The weights are the project's seeded state dict (oracle/seeded.py), as in
    tests/test_bbox_gpu.py: every parameter of the tail has a value, none is at its zero init."""
    import pairnet_amd as P
    from collections import OrderedDict
    from oracle import seeded
    head = P.CrossHeadBBox(**_cfg())
    if sd is None:
        sd = seeded.seeded_state_dict(
            OrderedDict((k, tuple(v.shape)) for k, v in head.state_dict().items()), seed)
    head.load_state_dict(sd)
    return head.to(DEV)


def _batch():
    g = torch.Generator().manual_seed(7)
    feats = [torch.randn(B, 256, h, w, generator=g).to(DEV) for h, w in SHAPES]
    metas = [dict(batch_input_shape=(H, W), img_shape=(H, W, 3), scale_factor=[1.0] * 4)] * B
    case = R.make_case(seed=11, G=(4, 6), T=(3, 7), num_classes=150, num_relations=50,
                       batch_shape=(H, W), planted=False)
    return feats, metas, case["gt_rels"], case["gt_bboxes"], case["gt_labels"]


@pytest.fixture(scope="module")
def setup(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    head = _head()
    feats, metas, gt_rels, gt_bboxes, gt_labels = _batch()
    return dict(head=head, sd=head.state_dict(), feats=feats, metas=metas, gt=(gt_rels, gt_bboxes,
                                                                               gt_labels))


def _oracle_tail(o, q, sub_pos, obj_pos):
    """oracle/bbox_head.py forward's tail (pairnet_bbox_head.py:268-320) with autograd ON, from the
    kept queries q [100, B, 256] and a given pair list."""
    bs = q.shape[1]
    s = F.normalize(o.sub_query_update(q).transpose(0, 1), p=2, dim=-1, eps=1e-12)
    ob = F.normalize(o.obj_query_update(q).transpose(0, 1), p=2, dim=-1, eps=1e-12)
    raw = torch.matmul(s, ob.transpose(1, 2))
    imp = o.update_importance(raw)
    take = lambda pos: torch.gather(q, 0, pos.unsqueeze(-1).repeat(1, 1, 256).transpose(0, 1))
    pair = torch.cat([take(sub_pos), take(obj_pos)], dim=0)
    rep = lambda e: e.weight.unsqueeze(1).repeat((1, bs, 1))
    rel_q, rel_q_pos = rep(o.rel_query_feat), rep(o.rel_query_pos_embed)
    rel_k_pos, rel_v_pos = rep(o.rel_key_pos_embed), rep(o.rel_value_pos_embed)
    for layer in o.relation_decoder.layers:
        rel_q = layer(query=rel_q, key=pair, value=pair, query_pos=rel_q_pos, key_pos=rel_k_pos,
                      value_pos=rel_v_pos, query_key_padding_mask=None, key_padding_mask=None)
    return dict(rel=o.rel_cls_embed(rel_q.transpose(0, 1)), importance=imp)


def test_tape_forward_and_gradients_against_the_oracle(setup):
    from oracle.bbox_head import OracleCrossHeadBBox
    from pairnet_amd import BBoxTailGrad
    head, feats, metas = setup["head"], setup["feats"], setup["metas"]
    gt_rels, gt_bboxes, gt_labels = setup["gt"]
    cls, box = head.forward(feats, metas)
    pl = head._last_plan
    want = {k: cls[k].clone() for k in ("rel", "importance", "sub", "obj")}
    tape = BBoxTailGrad(head)
    assert "rel_value_pos_embed.weight" not in tape.layout and "rel_key_pos_embed.weight" in tape.layout
    assert not any(k.startswith(("transformer.", "cls_branches", "reg_branches")) for k in tape.layout)
    q, kept_cls = pl.q.clone(), pl.cls.clone()
    out = tape.forward(q, kept_cls, pl.sub_pos, pl.obj_pos)
    torch.cuda.synchronize()
    for k in want:
        assert float((out[k] - want[k]).abs().max()) < 1e-4, k
    up = {}
    head.loss(dict(cls=kept_cls, sub=out["sub"], obj=out["obj"], rel=out["rel"],
                   importance=out["importance"]), dict(bbox=pl.box.clone()), gt_rels, gt_bboxes,
              gt_labels, metas, grads=up)
    assert set(up) == {"rel", "importance", "sub", "obj"}       # sub / obj: produced, unused
    dq, grads = tape.backward(g_rel=up["rel"], g_importance=up["importance"])
    torch.cuda.synchronize()
    assert dq is None and set(grads) == set(tape.layout)

    o = OracleCrossHeadBBox(**_cfg()).eval()
    o.load_state_dict({k: v.detach().cpu() for k, v in setup["sd"].items()}, strict=True)
    o = o.double()
    q_o = q.cpu().double().view(B, 100, 256).transpose(0, 1).contiguous()
    res = _oracle_tail(o, q_o, pl.sub_pos.cpu(), pl.obj_pos.cpu())
    sum((res[k] * up[k].cpu().double()).sum() for k in ("rel", "importance")).backward()
    ref = {k: p.grad for k, p in o.named_parameters() if p.grad is not None}
    report = []
    for k, g in grads.items():
        assert k in ref, k
        scale, err = float(ref[k].abs().max()), float((g.cpu().double() - ref[k]).abs().max())
        assert scale > 0.0, k
        report.append((err / scale, k, scale))
    moved = [k for k, g in ref.items() if float(g.abs().max()) > 0 and k not in grads]
    assert not moved, moved          # nothing the oracle differentiated is missing from the layout
    for r, k, scale in sorted(report, reverse=True)[:8]:
        print("%-64s relative error %.2e  (max |g| %.3e)" % (k, r, scale))
    worst = max(report)
    print("%d gradient tensors; worst relative error %.2e (%s)" % (len(grads), worst[0], worst[1]))
    assert worst[0] <= 1e-5, worst


def _trainer(sd, **kw):
    from pairnet_amd import BBoxTrainer
    head = _head(sd)
    return head, BBoxTrainer(head, **kw)


def test_step_first_update_frozen_parameters_and_write_back(setup):
    feats, metas, gt = setup["feats"], setup["metas"], setup["gt"]
    head, tr = _trainer(setup["sd"])
    p0 = tr.flat_p.clone()
    out = tr.step(feats, metas, *gt)
    torch.cuda.synchronize()
    assert set(out) == {"loss_r_cls", "loss_sub_cls", "loss_obj_cls", "loss_match", "grad_norm"}
    assert all(np.isfinite(float(v)) for v in out.values()) and float(out["grad_norm"]) > 0
    # the first update of every trained tensor = torch's AdamW + clip on the tape's own gradients
    gflat = tr.flat_grad.cpu().double()
    coef = min(1.0, tr.max_norm / (float(gflat.norm()) + 1e-6))
    lrs, wds = tr.seg_lr.cpu(), tr.seg_wd.cpu()
    worst = 0.0
    for i, (n, v) in enumerate(tr.params.items()):
        o, shape, k = tr.layout[n]
        p = p0[o:o + k].cpu().double().requires_grad_()
        opt = torch.optim.AdamW([p], lr=tr.lr * float(lrs[i]), weight_decay=tr.wd * float(wds[i]),
                                betas=tr.betas, eps=tr.eps)
        p.grad = gflat[o:o + k] * coef
        opt.step()
        worst = max(worst, float((v.reshape(-1).cpu().double() - p.detach()).abs().max()))
        assert float((v.reshape(-1) - p0[o:o + k]).abs().max()) > 0, n       # it moved
    print("first AdamW update: worst |difference| vs torch %.2e (lr %.0e)" % (worst, tr.lr))
    assert worst < 2e-2 * tr.lr
    # parameters outside the layout are bitwise unchanged, on the device and after write_back
    for k, v in head.w.items():
        if k in setup["sd"] and k not in tr.layout:
            assert torch.equal(v.cpu().reshape(-1), setup["sd"][k].reshape(-1)), k
    tr.write_back()
    sd1 = head.state_dict()
    for k, v in sd1.items():
        assert torch.equal(v, setup["sd"][k]) == (k not in tr.layout), k
    # inference through the trained head == a fresh head loaded from write_back()'s state dict
    a_cls, a_box = head.forward(feats, metas)
    a = {k: v.clone() for k, v in list(a_cls.items()) + list(a_box.items())}
    fresh = _head(sd1)
    b_cls, b_box = fresh.forward(feats, metas)
    torch.cuda.synchronize()
    for k, v in list(b_cls.items()) + list(b_box.items()):
        assert torch.equal(a[k], v), k


def test_two_runs_give_equal_bits_in_both_modes(setup):
    feats, metas, gt = setup["feats"], setup["metas"], setup["gt"]
    runs = []
    for mode in (False, False, True):
        head, tr = _trainer(setup["sd"], device_targets=mode)
        out = tr.step(feats, metas, *gt)
        out2 = tr.step(feats, metas, *gt)
        torch.cuda.synchronize()
        if mode:
            assert int(out["assign_status"]) == 0 and int(out2["assign_status"]) == 0
        runs.append((tr.flat_p.clone(), tr.flat_m.clone(), tr.flat_v.clone(),
                     {k: v.clone() for k, v in out2.items() if k != "assign_status"}))
    for other in runs[1:]:           # host twice, then device: the same bits
        for a, b in zip(runs[0][:3], other[:3]):
            assert torch.equal(a, b)
        for k, v in runs[0][3].items():
            assert torch.equal(v, other[3][k]), k


def test_planted_nan_skips_the_update_on_the_device(setup):
    feats, metas, gt = setup["feats"], setup["metas"], setup["gt"]
    head, tr = _trainer(setup["sd"], device_targets=True)
    tr.step(feats, metas, *gt)                       # (m and v are non-zero from here on)
    torch.cuda.synchronize()
    before = [t.clone() for t in (tr.flat_p, tr.flat_m, tr.flat_v)]
    # a NaN in one predicted box, planted behind the trunk's selection
    real = head._select

    def select_with_nan(pl):
        real(pl)
        pl.box[1, 17, 2] = float("nan")
    head._select = select_with_nan
    try:
        out = tr.step(feats, metas, *gt)
    finally:
        del head._select
    torch.cuda.synchronize()
    assert int(out["assign_status"]) != 0
    for a, b in zip(before, (tr.flat_p, tr.flat_m, tr.flat_v)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the same batch on the host path raises before any parameter moves, as scipy does
    head2, tr2 = _trainer(setup["sd"])
    real2 = head2._select

    def select_with_nan2(pl):
        real2(pl)
        pl.box[1, 17, 2] = float("nan")
    head2._select = select_with_nan2
    p0 = tr2.flat_p.clone()
    with pytest.raises(ValueError):
        tr2.step(feats, metas, *gt)
    torch.cuda.synchronize()
    assert torch.equal(p0, tr2.flat_p)


def test_detector_entry_points(setup):
    import pairnet_amd as P
    head, tr = _trainer(setup["sd"])
    det = P.PSGTr.__new__(P.PSGTr)
    det.bbox_head, det.neck, det.backbone = head, None, None
    feats, metas, gt = setup["feats"], setup["metas"], setup["gt"]
    det.extract_feat = lambda img: feats             # (a frozen backbone + neck's output)
    img = torch.zeros(B, 3, H, W, device=DEV)
    with pytest.raises(NotImplementedError):
        det.trainer()
    with pytest.raises(NotImplementedError):
        det.val_losses(img, metas, *gt)
    vals = det.val_box_losses(img, metas, *gt)
    assert set(vals) == {"loss_r_cls", "loss_sub_cls", "loss_obj_cls", "loss_match"}
    t = det.box_trainer(device_targets=True)
    assert isinstance(t, P.BBoxTrainer)
    out = det.box_train_step(img, metas, *gt)
    assert int(out["assign_status"]) == 0 and float(out["grad_norm"]) > 0
    res = det.box_train_step(dict(img=img, img_metas=metas, gt_rels=gt[0], gt_bboxes=gt[1],
                                  gt_labels=gt[2]), None)
    assert set(res) == {"loss", "log_vars", "num_samples"} and res["num_samples"] == B
