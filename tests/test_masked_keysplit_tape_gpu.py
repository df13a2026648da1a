"""GPU: `SegmenterHeadGrad.masked_keysplit_min_keys` -- the nine masked cross-attentions' backward
through `pn_mha_bwd_keysplit_masked_f32` -- under `tests/test_seg_grad_gpu.py`'s end-to-end
comparison (its `_reference`, `_compare`, `_compare_params`, `_trunk_names`, with their tolerances):
at that file's 64 x 96 pyramid (6 / 24 / 96 keys: every level inside one chunk) and at 128 x 192,
whose finest level has 384 keys, more than one chunk.  With the attribute at None the gradients are
bit for bit those of an untouched tape."""
import pytest
import torch

from helpers import baseline_cfg, oracle_baseline_head
from oracle import seeded
from test_grad_gpu import _compare, _compare_params, _print
from test_seg_grad_gpu import COUNTS, DEV, _reference, _train_cfg, _trunk_names

pytestmark = pytest.mark.gpu
_S = {}


def _setup(H, W):
    """(head, sd, pl, loss gradients) of one `return_all_layers=True` forward and the head's own
    segmentation losses; cached per image size."""
    if (H, W) not in _S:
        assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
        from pairnet_amd import CrossHeadBaseline
        _, sd, _ = oracle_baseline_head(1234)
        head = CrossHeadBaseline(**baseline_cfg(), train_cfg=_train_cfg())
        head.load_state_dict(sd)
        head.to(DEV)
        head.return_all_layers = True
        feats = seeded.seeded_feats(99, 2, H, W)
        metas = [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)] * 2
        cls, masks = head.forward([f.to(DEV) for f in feats], metas)
        gen = torch.Generator().manual_seed(8)
        gt_labels = [torch.randint(0, 133, (n,), generator=gen) for n in COUNTS]
        gt_masks = [(torch.rand(n, H // 2, W // 2, generator=gen) > 0.6).to(torch.uint8)
                    for n in COUNTS]
        grads = {}
        head.seg_losses(cls, masks, gt_labels, gt_masks, [dict()] * 2, grads=grads, seed=3)
        torch.cuda.synchronize()
        assert int(head.seg_status().cpu()) == 0
        _S[(H, W)] = (head, sd, head._last_plan, grads)
    return _S[(H, W)]


@pytest.mark.parametrize("H,W,finest", [(64, 96, 96), (128, 192, 384)])
def test_end_to_end_with_every_layer_on_the_masked_keysplit_kernel(H, W, finest):
    from pairnet_amd import SegmenterHeadGrad
    from pairnet_amd.hip import MHA_KEYSPLIT_CHUNK as c
    head, sd, pl, grads = _setup(H, W)
    assert max(pl.N) == finest and (finest > c) == (H == 128)
    tape = SegmenterHeadGrad(head)
    assert tape.masked_keysplit_min_keys is None
    tape.masked_keysplit_min_keys = 0
    tape.forward_from_plan(pl)
    calls = []
    from pairnet_amd import hip
    real = hip.mha_bwd_keysplit
    hip.mha_bwd_keysplit = lambda *a, **kw: (calls.append(kw), real(*a, **kw))[1]
    try:
        dmem, dMF, g = tape.backward(grads, counts=COUNTS)
    finally:
        hip.mha_bwd_keysplit = real
    torch.cuda.synchronize()
    assert len(calls) == 9 and all(kw["bits"] is not None and kw["rowall"] is not None
                                   for kw in calls)
    dmem_ref, dMF_ref, head_o = _reference(tape, pl, sd, grads)
    report = []
    _compare("memory tokens", dmem, dmem_ref, report)
    _compare("mask feature", dMF, dMF_ref, report)
    _compare_params(g, head_o, report, _trunk_names())
    _print(report)
    keep = (dmem.clone(), dMF.clone(), tape.flat_grad.clone())
    tape.forward_from_plan(pl)
    dmem2, dMF2, _ = tape.backward(grads, counts=COUNTS)       # reproducible bits
    assert torch.equal(dmem2, keep[0]) and torch.equal(dMF2, keep[1])
    assert torch.equal(tape.flat_grad, keep[2])


def test_threshold_selects_levels_and_none_is_the_untouched_tape():
    from pairnet_amd import SegmenterHeadGrad, hip
    head, sd, pl, grads = _setup(64, 96)
    plain = SegmenterHeadGrad(head)
    plain.forward_from_plan(pl)
    want = [t.clone() for t in plain.backward(grads, counts=COUNTS)[:2]] + [plain.flat_grad.clone()]
    tape = SegmenterHeadGrad(head)
    tape.forward_from_plan(pl)
    calls = []
    real = hip.mha_bwd_keysplit
    hip.mha_bwd_keysplit = lambda *a, **kw: (calls.append(a[10]), real(*a, **kw))[1]
    try:
        tape.masked_keysplit_min_keys = None
        got = list(tape.backward(grads, counts=COUNTS)[:2]) + [tape.flat_grad]
        assert calls == []
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        tape.masked_keysplit_min_keys = 1 << 30                 # above every level: the same
        tape.forward_from_plan(pl)
        got = list(tape.backward(grads, counts=COUNTS)[:2]) + [tape.flat_grad]
        assert calls == []
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        tape.masked_keysplit_min_keys = 24                      # the 24- and 96-key levels
        tape.forward_from_plan(pl)
        tape.backward(grads, counts=COUNTS)
        assert sorted(calls) == [24] * 3 + [96] * 3
    finally:
        hip.mha_bwd_keysplit = real
    for bad in (-1, 2.5, True, "0"):
        tape.masked_keysplit_min_keys = bad
        with pytest.raises(ValueError):
            tape.backward(grads, counts=COUNTS)


def test_baseline_tape_inherits_the_switch():
    from pairnet_amd import BaselineHeadGrad
    head, _, _, _ = _setup(64, 96)
    assert BaselineHeadGrad(head).masked_keysplit_min_keys is None
