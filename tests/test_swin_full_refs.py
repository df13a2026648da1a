"""CPU: (1) tests/swin_full_ref.py's float64 statements of the patch-merging + LayerNorm backward and
of the patch-embedding backward against autograd through oracle/swin.py's own PatchMerging /
PatchEmbed modules, at the maps of a 50 x 70 image (13x18: odd H, 7x9: both odd, 4x5: odd W);
(2) SwinStagesGrad's layout for frozen_stages in {-1, 0, 1, 2}: the trainable set of mmdet's
`_freeze_stages`, state-dict names, completion order, norm0 without learning rate or decay."""
import pytest
import torch

from oracle.swin import OracleSwin, PatchEmbed, PatchMerging, seeded_swin_state
from swin_full_ref import (BATCH, DIMS, IMG_H, IMG_W, frozen, patch_embed_bwd, patch_merge_ln_bwd,
                           to_neighbour_major, to_unfold)

TOL = 1e-10      # float64 against float64


def R(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _close(got, ref, what):
    scale = float(ref.abs().max())
    assert scale > 0 and float((got - ref).abs().max()) <= TOL * scale, what


@pytest.mark.parametrize("H,W,C", [(13, 18, 32), (7, 9, 64), (4, 5, 128), (1, 5, 32)])
def test_patch_merge_ln_bwd_statement_matches_autograd(H, W, C):
    B = BATCH
    pm = PatchMerging(C).double()
    with torch.no_grad():
        pm.norm.weight.copy_(R(4 * C, seed=1) * 0.3 + 1.0)
        pm.norm.bias.copy_(R(4 * C, seed=2) * 0.2)
        pm.reduction.weight.copy_(R(2 * C, 4 * C, seed=3) * (4 * C) ** -0.5)
    x = (R(B, H * W, C, seed=4) * 2.0 + 0.3).requires_grad_(True)
    out, (h2, w2) = pm(x, (H, W))
    assert (h2, w2) == ((H + 1) // 2, (W + 1) // 2)
    G = R(*out.shape, seed=5)
    (out * G).sum().backward()
    # d of the normalised rows, in the module's nn.Unfold order -> neighbour-major
    dy = to_neighbour_major((G @ pm.reduction.weight.detach()).reshape(-1, 4 * C), C)
    gamma = to_neighbour_major(pm.norm.weight.detach(), C)
    dx, dgamma, dbeta = patch_merge_ln_bwd(dy, x.detach().view(B, H, W, C), gamma, pm.norm.eps,
                                           B, H, W, C)
    _close(dx.view(B, H * W, C), x.grad, "dx")
    _close(to_unfold(dgamma, C), pm.norm.weight.grad, "d gamma")
    _close(to_unfold(dbeta, C), pm.norm.bias.grad, "d beta")
    # the two orders are each other's inverse
    assert torch.equal(to_unfold(to_neighbour_major(gamma, C), C), gamma)


def test_patch_embed_bwd_statement_matches_autograd():
    C = DIMS["embed_dims"]
    pe = PatchEmbed(C, 4).double()
    with torch.no_grad():
        pe.projection.weight.copy_(R(C, 3, 4, 4, seed=1) * 48 ** -0.5)
        pe.projection.bias.copy_(R(C, seed=2) * 0.1)
        pe.norm.weight.copy_(R(C, seed=3) * 0.3 + 1.0)
        pe.norm.bias.copy_(R(C, seed=4) * 0.2)
    img = R(BATCH, 3, IMG_H, IMG_W, seed=5)
    tok, hw = pe(img)
    assert hw == (13, 18)
    G = R(*tok.shape, seed=6)
    (tok * G).sum().backward()
    got = patch_embed_bwd(img, G.reshape(-1, C), pe.projection.weight.detach(),
                          pe.projection.bias.detach(), pe.norm.weight.detach(), pe.norm.eps)
    ref = dict(pe.named_parameters())
    for n, g in got.items():
        assert tuple(g.shape) == tuple(ref[n].shape), n
        _close(g, ref[n].grad, n)


# ---------------------------------------------------------------- layout
def _expected_groups(f, depths):
    nst, groups = len(depths), []
    for i in reversed(range(max(f, 0), nst)):
        if i < nst - 1:
            groups.append("stages.%d.downsample.reduction" % i)
        groups.append("norm%d" % i)
        if i < nst - 1:
            groups.append("stages.%d.downsample.norm" % i)
        groups += ["stages.%d.blocks.%d" % (i, j) for j in reversed(range(depths[i]))]
    if f < 0:
        groups.append("patch_embed")
    return groups


@pytest.mark.parametrize("f", [-1, 0, 1, 2])
def test_swin_stages_layout_is_the_reference_trainable_set(f):
    from pairnet_amd import SwinBackboneGrad, SwinStagesGrad, SwinTransformerHip
    from pairnet_amd.train import segment_multipliers
    swin = SwinTransformerHip(frozen_stages=f, **DIMS)
    sd = swin.state_dict()
    groups = SwinStagesGrad.param_groups(swin)
    names = [n for _, ns in groups for n in ns]
    want = {k for k in sd if not k.endswith("relative_position_index") and not frozen(k, f)}
    assert len(names) == len(set(names)) and set(names) == want
    assert set(names) <= set(sd)
    # what autograd reaches through the oracle under the same freeze (every map has a gradient)
    oracle = OracleSwin(**DIMS)
    oracle.load_state_dict(seeded_swin_state(oracle, 3))
    for n, p in oracle.named_parameters():
        p.requires_grad_(not frozen(n, f))
    g = torch.Generator().manual_seed(5)
    outs = OracleSwin.forward.__wrapped__(oracle, torch.randn(1, 3, IMG_H, IMG_W, generator=g))
    sum((o * torch.randn(o.shape, generator=g)).sum() for o in outs).backward()
    reached = {n for n, p in oracle.named_parameters()
               if p.grad is not None and float(p.grad.abs().max()) > 0}
    assert set(names) == reached
    # completion order: from the last stage down; per stage the merge's Linear, the output norm,
    # the merge's norm, the blocks last to first; the patch embedding at the very end
    assert [grp for grp, _ in groups] == _expected_groups(f, DIMS["depths"])
    assert SwinStagesGrad.size_of(swin) == sum((sd[n].numel() + 63) // 64 * 64 for n in names)
    # norm0: no gradient without d_c2 -> the trainer's segments give it lr 0 and wd 0
    assert SwinStagesGrad.NO_GRAD_GROUPS == ("norm0",)
    bb_names = ["backbone." + n for n in names]
    no_grad = {"backbone." + n for grp, ns in groups if grp in SwinStagesGrad.NO_GRAD_GROUPS
               for n in ns}
    assert no_grad == ({"backbone.norm0.weight", "backbone.norm0.bias"} if f <= 0 else set())
    for dm, wd_want in ((None, 1.0), ({"backbone.": 0.0}, 0.0)):
        lrs, wds = segment_multipliers(bb_names, no_grad, {"backbone.": 0.01}, dm, 0.0, swin=True)
        for n, lr, wd in zip(bb_names, lrs, wds):
            if n in no_grad:
                assert lr == 0.0 and wd == 0.0, n
            else:
                assert lr == 0.01 and wd == wd_want, n
    # the last-stage tape still refuses these values
    with pytest.raises(NotImplementedError):
        SwinBackboneGrad(swin)


def test_swin_stages_grad_refuses_the_last_stage_config():
    from pairnet_amd import SwinStagesGrad, SwinTransformerHip
    with pytest.raises(NotImplementedError):
        SwinStagesGrad(SwinTransformerHip(frozen_stages=3, **DIMS))
