"""CPU: the Swin backbone's trainable scope (SwinBackboneGrad.param_groups) is exactly what autograd
reaches through the oracle once mmdet's `_freeze_stages(3)` (configs/mask2former/pairnet_swinb.py:220,
frozen_stages=3) has frozen patch_embed, stages 0-2 with their patch merging, and norm0-norm2."""
import pytest
import torch

from oracle.swin import OracleSwin, seeded_swin_state

DIMS = dict(embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), window_size=7)


def _frozen(name, frozen_stages=3):
    """mmdet SwinTransformer._freeze_stages, restated: patch_embed, then for i in 1..frozen_stages
    stages[i - 1] (blocks AND downsample) and norm{i - 1}."""
    if name.startswith("patch_embed."):
        return True
    for i in range(1, frozen_stages + 1):
        if name.startswith("stages.%d." % (i - 1)) or name.startswith("norm%d." % (i - 1)):
            return True
    return False


def test_swin_grad_layout_is_the_reference_trainable_set():
    from pairnet_amd import SwinBackboneGrad, SwinTransformerHip
    oracle = OracleSwin(**DIMS)
    oracle.load_state_dict(seeded_swin_state(oracle, 3))
    for n, p in oracle.named_parameters():
        p.requires_grad_(not _frozen(n))
    g = torch.Generator().manual_seed(5)
    img = torch.randn(2, 3, 72, 100, generator=g)
    outs = OracleSwin.forward.__wrapped__(oracle, img)
    loss = sum((o * torch.randn(o.shape, generator=g)).sum() for o in outs)
    loss.backward()
    reached = {n for n, p in oracle.named_parameters()
               if p.grad is not None and float(p.grad.abs().max()) > 0}

    swin = SwinTransformerHip(frozen_stages=3, **DIMS)
    groups = SwinBackboneGrad.param_groups(swin)
    names = [n for _, ns in groups for n in ns]
    assert len(names) == len(set(names)) == 28
    assert set(names) == reached
    assert [grp for grp, _ in groups] == ["norm3", "stages.3.blocks.1", "stages.3.blocks.0"]
    assert not any(n.endswith("relative_position_index") for n in names)
    sd = swin.state_dict()
    assert SwinBackboneGrad.size_of(swin) == sum((sd[n].numel() + 63) // 64 * 64 for n in names)


def test_swin_backbone_keeps_training_settings_and_refuses_other_frozen_stages():
    from pairnet_amd import SwinBackboneGrad, SwinTransformerHip
    swin = SwinTransformerHip(frozen_stages=3, drop_path_rate=0.3, **DIMS)
    assert swin.frozen_stages == 3 and swin.drop_path_rate == 0.3
    plain = SwinTransformerHip(**DIMS)
    assert plain.frozen_stages == -1
    with pytest.raises(NotImplementedError):
        SwinBackboneGrad(plain)
    with pytest.raises(NotImplementedError):
        SwinBackboneGrad(SwinTransformerHip(frozen_stages=2, **DIMS))
