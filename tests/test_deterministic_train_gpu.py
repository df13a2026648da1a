"""GPU: `deterministic=True` from the pixel-decoder tape up to the trainers -- with the
deformable-attention backward summed without float atomics (`pn_msda_bwd_det_f32`) the tape's walk
and whole training steps are bitwise reproducible.  Fixtures of the existing trainer tests: seeded
heads (helpers, oracle.seeded), the 64 x 96 pyramid, batch 2."""
import pytest
import torch

from helpers import head_cfg, oracle_baseline_head, oracle_head
from oracle import seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 64, 96
TOL = 1e-4                   # tests/test_grad_gpu.py's: of each tensor's largest entry


def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


def _walk(tape, *upstream, **kw):
    dfeats, grads = tape.backward(*upstream, **kw)
    torch.cuda.synchronize()
    return [None if d is None else d.clone() for d in dfeats], {k: v.clone() for k, v in grads.items()}


def _assert_equal_walks(a, b):
    assert len(a[0]) == len(b[0]) and sorted(a[1]) == sorted(b[1])
    for l, (x, y) in enumerate(zip(a[0], b[0])):
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), "features %d" % l
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), n


def _assert_close_walks(a, b):
    worst = 0.0
    pairs = [("features %d" % l, x, y) for l, (x, y) in enumerate(zip(a[0], b[0])) if x is not None]
    pairs += [(n, a[1][n], b[1][n]) for n in a[1]]
    for n, x, y in pairs:
        scale, err = float(y.abs().max()), float((x - y).abs().max())
        worst = max(worst, err / scale if scale else 0.0)
        assert err <= TOL * scale, (n, err, scale)
    return worst


def test_pixel_decoder_tapes_walk_is_bitwise_reproducible():
    """`SegPixelDecoderGrad` (117 gradients, d C5 / C4 / C3 / C2) and its parent `PixelDecoderGrad`
    (109): two `backward` on one forward are `torch.equal` throughout with `deterministic = True`,
    and within 1e-4 of each tensor's largest entry of the atomic walk."""
    _need_gpu()
    from pairnet_amd import PixelDecoderGrad, SegPixelDecoderGrad
    from test_baseline_train_gpu import _head
    _, sd, _ = oracle_baseline_head(1234)
    head = _head(sd)
    feats = [f.to(DEV) for f in seeded.seeded_feats(99, 2, H, W)]
    tape = SegPixelDecoderGrad(head)
    assert tape.deterministic is False and tape.msda_scratch is None
    mem, MF = tape.forward(feats)
    g = torch.Generator().manual_seed(21)
    G_mem = torch.randn(tuple(mem.shape), generator=g).to(DEV)
    G_MF = torch.randn(tuple(MF.shape), generator=g).to(DEV)
    atomic = _walk(tape, G_mem, G_MF, need_dc2=True)
    assert tape.msda_scratch is None                       # the default never allocates it
    tape.deterministic = True
    first = _walk(tape, G_mem, G_MF, need_dc2=True)
    scratch = tape.msda_scratch
    assert scratch is not None and scratch.dtype == torch.uint8
    second = _walk(tape, G_mem, G_MF, need_dc2=True)
    assert tape.msda_scratch is scratch                    # one tensor, six layers, every call
    assert len(first[1]) == 117 and sum(d is not None for d in first[0]) == 4
    _assert_equal_walks(first, second)
    print("SegPixelDecoderGrad: deterministic vs atomic walk, worst err / max = %.2e"
          % _assert_close_walks(first, atomic))

    parent = PixelDecoderGrad(head)
    parent.deterministic = True
    parent.forward(feats)
    p1 = _walk(parent, G_mem)
    p2 = _walk(parent, G_mem)
    assert len(p1[1]) == 109 and len(p1[0]) == 3
    _assert_equal_walks(p1, p2)
    parent.deterministic = False
    print("PixelDecoderGrad: deterministic vs atomic walk, worst err / max = %.2e"
          % _assert_close_walks(p1, _walk(parent, G_mem)))


def _tail_batch():
    g = torch.Generator().manual_seed(2)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[2.0] * 4)] * 2
    gt_labels = [torch.tensor([3, 17, 90, 120, 3]), torch.tensor([5, 60, 7])]
    gt_masks = [torch.rand(5, H, W, generator=g) > 0.6, torch.rand(3, H, W, generator=g) > 0.5]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 3, 17], [1, 0, 56], [4, 2, 5], [0, 1, 9]]),
               torch.tensor([[0, 1, 2], [2, 1, 30]])]
    pts = [torch.rand(1, 12544, 2, generator=g) for _ in range(2)]
    return metas, gt_rels, gt_labels, gt_masks, pts


def _tail_head(sd):
    from pairnet_amd import CrossHead2
    head = CrossHead2(**head_cfg())
    head.load_state_dict(sd)
    return head.to(DEV)


def _two_steps(tr, step):
    """Two steps -> every returned value of both, and the trainer's state."""
    vals = []
    for _ in range(2):
        out = step()
        torch.cuda.synchronize()
        vals.append({k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in out.items()})
    state = {k: getattr(tr, k).clone() for k in ("flat_p", "flat_m", "flat_v", "clip")}
    return vals, state


def _assert_same_run(a, b):
    for va, vb in zip(a[0], b[0]):
        assert sorted(va) == sorted(vb)
        for k in va:
            same = torch.equal(va[k], vb[k]) if isinstance(va[k], torch.Tensor) else va[k] == vb[k]
            assert same, "returned %s" % k
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("scope", ["pixel_decoder", "resnet"])
def test_tail_trainer_steps_are_bitwise_reproducible(scope):
    """Two `TailTrainer(..., deterministic=True)` on two heads of one state dict, two steps each on
    the same batch: parameters, both moments, the clip record and every returned value are
    `torch.equal`.  "resnet": + a ResNet-50's stages 2-4, from the image."""
    _need_gpu()
    from pairnet_amd import ResNet50Hip, TailTrainer
    _, sd, _ = oracle_head(1234)
    metas, gt_rels, gt_labels, gt_masks, pts = _tail_batch()
    if scope == "resnet":
        x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(5)).to(DEV)
        bsd = ResNet50Hip().state_dict()
    else:
        x = [f.to(DEV) for f in seeded.seeded_feats(99, 2, H, W)]
    runs = []
    for _ in range(2):
        bb = None
        if scope == "resnet":
            bb = ResNet50Hip()
            bb.load_state_dict(bsd)
            bb.to(DEV)
        tr = TailTrainer(_tail_head(sd), lr=1e-3, train_pixel_decoder=True, backbone=bb,
                         deterministic=True)
        assert tr.pd_tape.deterministic is True
        runs.append(_two_steps(tr, lambda: tr.step(x, metas, gt_rels, gt_labels, gt_masks,
                                                   point_coords=pts)))
        assert tr.pd_tape.msda_scratch is not None
    assert float(runs[0][0][1]["grad_norm"]) > 0
    _assert_same_run(runs[0], runs[1])


def test_baseline_trainer_steps_are_bitwise_reproducible():
    _need_gpu()
    from pairnet_amd import BaselineTrainer
    from test_baseline_train_gpu import SEED, _batch, _head
    _, sd, _ = oracle_baseline_head(1234)
    metas, gt_rels, gt_labels, gt_masks = _batch()
    x = [f.to(DEV) for f in seeded.seeded_feats(99, 2, H, W)]
    runs = []
    for _ in range(2):
        tr = BaselineTrainer(_head(sd), lr=1e-3, seed=SEED, deterministic=True)
        assert tr.pd_tape.deterministic is True
        runs.append(_two_steps(tr, lambda: tr.step(x, metas, gt_rels, gt_labels, gt_masks)))
    assert float(runs[0][0][1]["grad_norm"]) > 0
    _assert_same_run(runs[0], runs[1])


def test_keyword_without_a_pixel_decoder_tape_changes_nothing():
    """`TailTrainer(head, deterministic=True)` has no pixel-decoder tape: it steps bit for bit like
    the default trainer.  A default trainer WITH the tape never allocates the scratch."""
    _need_gpu()
    from pairnet_amd import TailTrainer
    _, sd, _ = oracle_head(1234)
    metas, gt_rels, gt_labels, gt_masks, pts = _tail_batch()
    x = [f.to(DEV) for f in seeded.seeded_feats(99, 2, H, W)]
    runs = []
    for kw in (dict(), dict(deterministic=True)):
        tr = TailTrainer(_tail_head(sd), lr=1e-3, **kw)
        assert tr.pd_tape is None
        runs.append(_two_steps(tr, lambda: tr.step(x, metas, gt_rels, gt_labels, gt_masks,
                                                   point_coords=pts)))
    _assert_same_run(runs[0], runs[1])
    tr = TailTrainer(_tail_head(sd), lr=1e-3, train_pixel_decoder=True)
    assert tr.deterministic is False and tr.pd_tape.deterministic is False
    tr.step(x, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
    torch.cuda.synchronize()
    assert tr.pd_tape.msda_scratch is None
