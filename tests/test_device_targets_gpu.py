"""GPU: `device_targets=True` -- loss targets built on the device (csrc/assign.hip: the Hungarian
assignments and the bookkeeping of `_get_target_single`), no host wait in `CrossHead2.loss` or
`TailTrainer.step` -- against the default host path on the 96 x 128 fixture of
tests/test_losses_gpu.py, batch 2 (its relations [0,1,5] / [0,1,9] share a class pair: a tie).
The same kernels read the same targets, so every comparison is bitwise."""
import numpy as np
import pytest
import torch

from helpers import head_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, BS = 96, 128, 2
TERMS = ("loss_r_cls", "loss_sub_cls", "loss_obj_cls", "loss_match")


def _head():
    from pairnet_amd import CrossHead2
    head = CrossHead2(**head_cfg())
    head.init_weights(seed=3)
    return head.to(DEV)


def _batch(seed=2):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(BS, c, H // s, W // s, generator=g).to(DEV)
             for c, s in zip((256, 512, 1024, 2048), (4, 8, 16, 32))]
    metas = [dict(img_shape=(H, W, 3), scale_factor=[2.0] * 4)] * BS
    gt_labels = [torch.tensor([3, 17, 90, 120, 3]), torch.tensor([5, 60, 7])]
    gt_masks = [torch.rand(5, H, W, generator=g) > 0.6, torch.rand(3, H, W, generator=g) > 0.5]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 3, 17], [1, 0, 56], [4, 2, 5], [0, 1, 9]]),
               torch.tensor([[0, 1, 2], [2, 1, 30]])]
    pts = [torch.rand(1, 12544, 2, generator=g) for _ in range(BS)]
    return feats, metas, gt_rels, gt_labels, gt_masks, pts


@pytest.fixture(scope="module")
def outputs():
    """One head, its outputs on the fixture batch (shared, never written)."""
    head = _head()
    feats, metas, gt_rels, gt_labels, gt_masks, pts = _batch()
    cls, masks = head.forward(feats, metas)
    cls = {k: v.clone() for k, v in cls.items()}
    masks = {k: v.clone() for k, v in masks.items()}
    return head, cls, masks, metas, gt_rels, gt_labels, gt_masks, pts


def _loss_object(head):
    from pairnet_amd.losses import CrossHead2Loss
    return CrossHead2Loss(head.num_classes, head.num_relations, head.num_obj_query,
                          head.num_rel_query, **head._loss_cfg)


def _no_host_wait(monkeypatch):
    """Every way this code base has of waiting for the device raises."""
    from pairnet_amd import losses

    def refuse(name):
        def f(*a, **kw):
            raise AssertionError("host wait: " + name)
        return f
    monkeypatch.setattr(losses, "linear_sum_assignment", refuse("linear_sum_assignment"))
    for name in ("cpu", "item", "numpy", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, refuse("Tensor." + name))


def test_device_targets_equal_host_targets_bitwise(outputs):
    head, cls, masks, metas, gt_rels, gt_labels, gt_masks, pts = outputs
    res = {}
    for mode in (False, True):
        lo = _loss_object(head)
        trace, grads = [], {}
        first = lo.loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, point_coords=pts,
                        trace=trace, grads=grads, device_targets=mode)
        first = {k: v.clone() for k, v in first.items()}
        cum1 = lo.cum_samples.copy()
        second = lo.loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, point_coords=pts,
                         device_targets=mode)
        res[mode] = dict(first=first, second=second, trace=trace, grads=grads, cum1=cum1,
                         cum2=lo.cum_samples.copy(), on_device=lo.last_on_device,
                         status=lo.assign_status)
    host, dev = res[False], res[True]
    assert dev["on_device"] and not host["on_device"]
    assert int(dev["status"].cpu()[0]) == 0
    assert set(dev["first"]) == set(TERMS)
    for k in TERMS:
        print(k, float(host["first"][k]), float(dev["first"][k]))
        assert torch.equal(host["first"][k], dev["first"][k]), k
        assert torch.equal(host["second"][k], dev["second"][k]), k
    assert set(dev["grads"]) == {"rel", "sub", "obj", "importance"}
    for k, g in host["grads"].items():
        assert torch.equal(g, dev["grads"][k]), k
    assert len(dev["trace"]) == len(host["trace"]) == BS
    for a, b in zip(host["trace"], dev["trace"]):
        assert set(a) == set(b)
        for k in ("mask_rows", "mask_cols", "triplet_rows", "triplet_cols"):
            assert np.array_equal(a[k], b[k]), k
        for k in ("mask_cost", "id_cost", "pred_pts", "gt_pts"):
            assert torch.equal(a[k].cpu(), b[k].cpu()), k
    # SeesawLoss's counts: equal after one and after two calls, and they weigh the second call
    assert np.array_equal(host["cum1"], dev["cum1"]) and host["cum1"].sum() == 7
    assert np.array_equal(host["cum2"], dev["cum2"]) and host["cum2"].sum() == 14
    assert float(dev["second"]["loss_r_cls"]) != float(dev["first"]["loss_r_cls"])


def test_head_loss_passes_the_switch_through(outputs):
    head, cls, masks, metas, gt_rels, gt_labels, gt_masks, pts = outputs
    head._loss = None
    a = head.loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, point_coords=pts,
                  device_targets=True)
    assert head._loss.last_on_device
    want = _loss_object(head).loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas,
                                   point_coords=pts)
    for k in TERMS:
        assert torch.equal(a[k], want[k]), k
    head._loss = None


def test_device_mode_never_waits_for_the_host(outputs, monkeypatch):
    from pairnet_amd import TailTrainer
    head, cls, masks, metas, gt_rels, gt_labels, gt_masks, pts = outputs
    feats = _batch()[0]
    trainer = TailTrainer(_head(), device_targets=True)
    lo_dev, lo_host = _loss_object(head), _loss_object(head)
    with monkeypatch.context() as m:
        _no_host_wait(m)
        # the check can see a wait: the default mode trips it
        with pytest.raises(AssertionError, match="host wait"):
            lo_host.loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, point_coords=pts)
        got = lo_dev.loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, point_coords=pts,
                          grads={}, device_targets=True)
        # (default points: torch.rand on the device, no wait either)
        lo_dev.loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, device_targets=True)
        out = trainer.step(feats, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(got[k])) for k in TERMS)
    assert int(out["assign_status"]) == 0 and np.isfinite(float(out["grad_norm"]))
    # torch's own detector of synchronising calls, where this build's flags the default mode's
    # blocking copies (labnotes/r11.md says what it did on the MI355X stack)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            lo_host.loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, point_coords=pts)
            flagged = False
        except RuntimeError as e:
            flagged = "synchroniz" in str(e)
            if not flagged:
                raise
        print("set_sync_debug_mode('error') flags the default mode:", flagged)
        if flagged:
            lo_dev.loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, point_coords=pts,
                        grads={}, device_targets=True)
            trainer.step(feats, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dropout,steps", [(False, 3), (True, 1)])
def test_two_trainers_stay_bitwise_equal(dropout, steps):
    from pairnet_amd import TailTrainer
    feats, metas, gt_rels, gt_labels, gt_masks, pts = _batch()
    ref = _head()
    sd = ref.state_dict()
    runs = []
    for mode in (False, True):
        head = _head()
        head.load_state_dict(sd)
        head.to(DEV)
        tr = TailTrainer(head, lr=1e-3, seed=5, dropout=dropout, device_targets=mode)
        assert tr.device_targets is mode and not tr.train_decoder
        losses = []
        for _ in range(steps):
            out = tr.step(feats, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
            losses.append({k: v.clone() for k, v in out.items()})
        runs.append((tr, losses))
    (host, lh), (dev, ld) = runs
    assert "assign_status" not in lh[0] and all(int(o["assign_status"]) == 0 for o in ld)
    for a, b in zip(lh, ld):
        for k in TERMS + ("grad_norm",):
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(host.flat_p, dev.flat_p)
    assert torch.equal(host.flat_m, dev.flat_m) and torch.equal(host.flat_v, dev.flat_v)
    assert np.array_equal(host.head._loss.cum_samples, dev.head._loss.cum_samples)
    assert host.steps == dev.steps == steps


def test_a_refused_cost_matrix_moves_no_parameter():
    """One NaN among the mask logits: scipy raises on the host path before any parameter moves;
    the device path reports it in `assign_status` and its guarded AdamW launch returns early."""
    from pairnet_amd import TailTrainer
    feats, metas, gt_rels, gt_labels, gt_masks, pts = _batch()
    head = _head()
    tr = TailTrainer(head, lr=1e-3, device_targets=True)
    tr.step(feats, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)     # (non-zero m, v)
    before = [t.clone() for t in (tr.flat_p, tr.flat_m, tr.flat_v)]
    cum = head._loss.cum_samples.copy()
    forward = head.forward

    def poisoned(*a, **kw):
        cls, masks = forward(*a, **kw)
        masks["mask"][1, 7, 3, 5] = float("nan")
        return cls, masks
    head.forward = poisoned
    try:
        out = tr.step(feats, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
    finally:
        del head.forward
    assert int(out["assign_status"]) == 1
    for a, b in zip(before, (tr.flat_p, tr.flat_m, tr.flat_v)):
        assert torch.equal(a, b)
    assert np.array_equal(head._loss.cum_samples, cum)
    assert tr.steps == 2              # the host counter advances all the same (documented)
    # the host path's guarantee, for comparison: it raises
    with pytest.raises(ValueError):
        cls, masks = poisoned(feats, metas)
        head.loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas, point_coords=pts)
    # the next clean step works
    out = tr.step(feats, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
    assert int(out["assign_status"]) == 0
    assert all(np.isfinite(float(out[k])) for k in TERMS + ("grad_norm",))
    assert not torch.equal(before[0], tr.flat_p) and bool(torch.isfinite(tr.flat_p).all())


def test_counts_survive_a_state_dict_round_trip_across_modes(outputs):
    head, cls, masks, metas, gt_rels, gt_labels, gt_masks, pts = outputs
    call = lambda lo, mode: lo.loss(cls, masks, gt_rels, None, gt_labels, gt_masks, metas,
                                    point_coords=pts, device_targets=mode)
    host = _loss_object(head)
    call(host, False)
    want = call(host, False)
    a = _loss_object(head)
    call(a, True)
    sd = a.state_dict()
    assert set(sd) == set(host.state_dict()) == {"rel_cls_loss.cum_samples"}
    assert isinstance(sd["rel_cls_loss.cum_samples"], torch.Tensor) and not sd["rel_cls_loss.cum_samples"].is_cuda
    b = _loss_object(head)
    b.load_state_dict(sd)
    got = call(b, False)                         # device counts -> state dict -> host mode
    assert np.array_equal(b.cum_samples, host.cum_samples)
    assert torch.equal(got["loss_r_cls"], want["loss_r_cls"])
    c = _loss_object(head)
    call(c, False)
    d = _loss_object(head)
    d.load_state_dict(c.state_dict())
    got = call(d, True)                          # host counts -> state dict -> device mode
    assert np.array_equal(d.cum_samples, host.cum_samples)
    assert torch.equal(got["loss_r_cls"], want["loss_r_cls"])
    e = _loss_object(head)                       # one object switching modes between calls
    call(e, True)
    got = call(e, False)
    assert torch.equal(got["loss_r_cls"], want["loss_r_cls"])
    assert isinstance(e.cum_samples, np.ndarray) and np.array_equal(e.cum_samples, host.cum_samples)
