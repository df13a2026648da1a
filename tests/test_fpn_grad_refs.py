"""CPU: the float64 statements of tests/fpn_grad_ref.py pinned to torch and to the reference-pinned
oracle, the conditions tests/test_fpn_grad_kernels_gpu.py / tests/test_fpn_grad_gpu.py rely on (the
ReLU-gate cap under an fp32 run, the integer case being exact), and the new surface's boundary:
header, bindings, exports, layout."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import fpn_grad_ref as R
from helpers import baseline_cfg, oracle_baseline_head
from oracle import seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1, 1, 1), (1, 1, 3, 5), (5, 5, 5, 5), (8, 12, 16, 24), (7, 10, 13, 19), (3, 4, 5, 7),
         (2, 3, 9, 4)]
PYRAMIDS = [(64, 96), (52, 76)]
_S = {}


def _pixel_decoder():
    if "pd" not in _S:
        head, sd, _ = oracle_baseline_head(1234)
        _S["pd"] = head.double().pixel_decoder
    return _S["pd"]


def _oracle_run(H, W):
    if (H, W) not in _S:
        pd = _pixel_decoder()
        feats = [f.double() for f in seeded.seeded_feats(99, 2, H, W)]
        with torch.no_grad():
            mf, outs = pd(feats)
        _S[(H, W)] = (feats, mf, outs)
    return _S[(H, W)]


@pytest.mark.parametrize("hi,wi,ho,wo", SIZES)
def test_adjoint_statement_is_autograd_of_interpolate(hi, wi, ho, wo):
    g = torch.Generator().manual_seed(hi * 100 + wo)
    x = torch.randn(2, 3, hi, wi, generator=g, dtype=torch.float64, requires_grad=True)
    G = torch.randn(2, 3, ho, wo, generator=g, dtype=torch.float64)
    y = F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=False)
    ref, = torch.autograd.grad(y, x, G)
    d, mag, extra = R.bilinear_adjoint(G, hi, wi)
    assert float((d - ref).abs().max()) <= 1e-12
    assert bool((mag >= d.abs() - 1e-12).all()) and bool((extra >= 0).all())
    # the forward is the same matrices, and every fine index that taps i lies in i's window
    Ty, Tx = R.tap_matrix(hi, ho), R.tap_matrix(wi, wo)
    assert float((torch.einsum("oi,...ij,pj->...op", Ty, x.detach(), Tx) - y.detach()).abs().max()) <= 1e-12
    for T, W in ((Ty, R.window_matrix(hi, ho)), (Tx, R.window_matrix(wi, wo))):
        assert bool(((T != 0) <= (W != 0)).all())
        assert float((T.sum(1) - 1.0).abs().max()) <= 1e-12       # rows of a resampling sum to 1
    if (hi, wi) == (ho, wo):
        assert torch.equal(d, G)                                  # identity


def test_exact_two_times_has_at_most_four_contributors_and_integer_taps():
    assert R.adjoint_contributors(8, 16) <= 6 and R.adjoint_contributors(12, 24) <= 6
    T = R.tap_matrix(8, 16)
    assert int((T != 0).sum(0).max()) <= 4
    # every weight is a multiple of 1/4: with small integer g the adjoint is exact in fp32, in any
    # summation order (what the GPU file's integer case compares bit for bit)
    assert torch.equal(T * 4, (T * 4).round())
    g = torch.randint(-8, 9, (2, 4, 16, 24), generator=torch.Generator().manual_seed(3)).double()
    d, _, _ = R.bilinear_adjoint(g, 8, 12)
    assert torch.equal(d * 16, (d * 16).round()) and float(d.abs().max()) < 2 ** 10
    assert torch.equal(d.float().double(), d)


def test_src_is_an_integer_at_row_6_of_7_to_13():
    """13 rows over 7: src = 7 / 13 * 6.5 - 0.5 = 3 exactly in real arithmetic -- the case where an
    fp32 floor may fall either side; the row lies in the windows of coarse rows 2, 3 and 4."""
    from fractions import Fraction
    assert Fraction(7, 13) * Fraction(13, 2) - Fraction(1, 2) == 3
    for i in (2, 3, 4):
        lo, hi = R.window(i, 7, 13)
        assert lo <= 6 <= hi


@pytest.mark.parametrize("G,relu", [(32, False), (32, True), (4, True)])
def test_group_norm_backward_statement_is_autograd(G, relu):
    g = torch.Generator().manual_seed(G + relu)
    B, HW, C = 2, 37, 256
    x = torch.randn(B, HW, C, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, HW, C, generator=g, dtype=torch.float64)
    y = F.group_norm(x.permute(0, 2, 1), G, gamma, beta, 1e-5).permute(0, 2, 1)
    out = F.relu(y) if relu else y
    dx, dg, db = torch.autograd.grad(out, (x, gamma, beta), dy)
    gate = (y.detach() > 0).double() if relu else None
    s = R.group_norm_bwd(x.detach(), dy, gamma.detach(), G, 1e-5, gate)
    for k, ref in (("dx", dx), ("dgamma", dg), ("dbeta", db)):
        assert float((s[k] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), k
        assert bool((s[k + "_mag"] >= s[k].abs() * (1 - 1e-12)).all()), k


@pytest.mark.parametrize("H,W", PYRAMIDS)
def test_branch_statement_is_the_oracles_mask_feature(H, W):
    feats, mf, outs = _oracle_run(H, W)
    p = R.branch_params(_pixel_decoder())
    assert sorted(p) == sorted(R.BRANCH_PARAMS)
    with torch.no_grad():
        mine, z = R.branch(feats[0], outs[2], p, baseline_cfg_groups())
        assert float((mine - mf).abs().max()) <= 1e-12
        # an external gate equal to the statement's own sign changes nothing
        gated, _ = R.branch(feats[0], outs[2], p, baseline_cfg_groups(), gate=(z > 0).double())
        assert float((gated - mf).abs().max()) <= 1e-12


def baseline_cfg_groups():
    return baseline_cfg()["pixel_decoder"]["norm_cfg"]["num_groups"]


@pytest.mark.parametrize("H,W", PYRAMIDS)
def test_relu_gate_of_an_fp32_run_stays_inside_the_cap(H, W):
    """The condition the GPU comparison rests on: an fp32 evaluation's gate (z > 0) differs from the
    float64 statement's on at most 0.1 % of the elements at these seeds."""
    feats, mf, outs = _oracle_run(H, W)
    p = R.branch_params(_pixel_decoder())
    with torch.no_grad():
        _, z64 = R.branch(feats[0], outs[2], p, baseline_cfg_groups())
        _, z32 = R.branch(feats[0].float(), outs[2].float(), {k: v.float() for k, v in p.items()},
                          baseline_cfg_groups())
    frac = R.gate_mismatch((z32 > 0).float(), z64)
    print("gate mismatch fp32 vs float64 at %dx%d: %.3e (cap %.0e)" % (H, W, frac, R.GATE_CAP))
    assert frac <= R.GATE_CAP


def test_new_entries_are_declared_bound_and_exported():
    from pairnet_amd import CrossHeadBaseline, SegPixelDecoderGrad, api, hip
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    for name in ("pn_bilinear_nhwc_bwd_f32", "pn_groupnorm_act_nhwc_bwd_f32"):
        assert name in declared and name in hip._SIGS and name in hip.EXPORTS, name
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION
    assert callable(hip.bilinear_nhwc_bwd) and callable(hip.groupnorm_act_nhwc_bwd)
    assert SegPixelDecoderGrad.__name__ in api.__all__
    assert hasattr(CrossHeadBaseline, "segmenter_backward")


def test_layout_puts_the_three_new_groups_first():
    from pairnet_amd import CrossHeadBaseline, PixelDecoderGrad, SegPixelDecoderGrad
    head = CrossHeadBaseline(**baseline_cfg())
    groups = SegPixelDecoderGrad.param_groups(head)
    assert [g for g, _ in groups[:3]] == ["mask_feature", "output_convs.0", "lateral_convs.0"]
    assert groups[0][1] == R.BRANCH_PARAMS[:2] and groups[1][1] == R.BRANCH_PARAMS[2:5]
    assert groups[2][1] == R.BRANCH_PARAMS[5:]
    assert groups[3:] == PixelDecoderGrad.param_groups(head)
    names = [n for _, ns in groups for n in ns]
    assert len(names) == len(set(names)) == 117
    assert sorted(names) == sorted(k for k in head.param_shapes() if k.startswith("pixel_decoder."))
    extra = sum((int(torch.Size(head.param_shapes()[n]).numel()) + 63) // 64 * 64
                for n in R.BRANCH_PARAMS)
    assert SegPixelDecoderGrad.size_of(head) == PixelDecoderGrad.size_of(head) + extra
    with pytest.raises(RuntimeError):
        SegPixelDecoderGrad(head)                                    # not on the device
