"""CPU: the statements tests/test_grouped_conv_gpu.py compares the grouped convolution and the
ResNeXt backbone with (tests/grouped_conv_ref.py) against torch in float64, on that test's own
cases; the ResNeXt state-dict layout; the reference's pairnet_rnext101_vg.py dropping in; the
refusals that need no device (unsupported group widths, trainers over a forward-only backbone);
the boundary (header, bindings, ABI)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import grouped_conv_ref as GR
import mm_ref as R
from oracle import ref_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pn_conv2d_grouped_nhwc_f32"


def _torch64(x, w, bias, G, stride, relu):
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), stride=stride,
                 padding=1, groups=G).permute(0, 2, 3, 1)
    return F.relu(y) if relu else y


@pytest.mark.parametrize("ci", range(len(GR.CASES)))
def test_statement_equals_torch_float64(ci):
    c = GR.CASES[ci]
    B, H, W, G, Cg, s = c
    for operands in (GR.exact_operands, GR.random_operands):
        x, w, bias = operands(c, 300 + ci)
        ref, mag = GR.grouped_conv(x, w, bias, G, s, GR.relu_of(ci))
        want = _torch64(x, w, bias, G, s, GR.relu_of(ci))
        assert ref.shape == want.shape == (B,) + GR.out_hw(H, W, s) + (G * Cg,)
        assert float((ref - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        wantm = _torch64(x.abs(), w.abs(), bias.abs(), G, s, False)
        assert float((mag - wantm).abs().max()) <= 1e-12 * float(wantm.abs().max())


@pytest.mark.parametrize("ci", range(len(GR.CASES)))
def test_integer_cases_are_exact_in_fp32(ci):
    """mag = sum |x| |w| + |bias| bounds every partial sum in any order: below 2^24 all of them are
    integers fp32 holds exactly, so the kernel must return the statement bit for bit."""
    c = GR.CASES[ci]
    x, w, bias = GR.exact_operands(c, 300 + ci)
    ref, mag = GR.grouped_conv(x, w, bias, c[3], c[5], GR.relu_of(ci))
    assert float(mag.max()) < R.EXACT
    assert torch.equal(ref, ref.round()) and torch.equal(ref.float().double(), ref)
    assert len(set(bias.tolist())) == bias.numel()          # distinct per channel


def test_cases_cover_what_the_kernel_branches_on():
    cs = set(GR.CASES)
    for c in [(2, 7, 9, 32, 8, 1), (1, 9, 11, 32, 16, 2), (1, 6, 5, 32, 32, 1),
              (1, 5, 7, 32, 64, 2), (1, 1, 1, 1, 8, 1), (1, 2, 3, 3, 8, 2), (2, 8, 8, 5, 16, 2)]:
        assert c in cs
    for Cg in (8, 16, 32, 64):
        per_wg = GR.WG_CHANNELS // Cg
        for s in (1, 2):
            # one more than the pixel tile on both sides of the OUTPUT map
            assert any(c[4] == Cg and c[5] == s and
                       GR.out_hw(c[1], c[2], s) == (GR.TILE_H[s] + 1, GR.TILE_W + 1) for c in cs)
        if per_wg > 1:
            assert any(c[4] == Cg and c[3] % per_wg and c[3] > per_wg for c in cs)
    s2 = [(c, GR.relu_of(i)) for i, c in enumerate(GR.CASES) if c[5] == 2]
    for parity in (0, 1):
        for relu in (False, True):
            assert any(c[1] % 2 == parity and c[2] % 2 == parity and r == relu for c, r in s2), \
                (parity, relu)


@pytest.mark.parametrize("depth", [50, 101])
def test_state_dict_layout(depth):
    from pairnet_amd import ResNeXtHip
    net = ResNeXtHip(depth, 32, 8)
    ours = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert ours == [(k, tuple(s)) for k, s in GR.param_shapes(depth, 32, 8).items()]
    sd = dict(ours)
    for i, (wd, blocks) in enumerate(zip((256, 512, 1024, 2048), GR.BLOCKS[depth])):
        assert net.widths[i] == wd
        for b in (0, blocks - 1):
            assert sd["layer%d.%d.conv2.weight" % (i + 1, b)] == (wd, wd // 32, 3, 3)
            assert sd["layer%d.%d.conv3.weight" % (i + 1, b)] == (64 * 2 ** i * 4, wd, 1, 1)
    # a seeded state of the restatement loads, strictly
    if depth == 50:
        net.load_state_dict(GR.seeded_state(3, 50))


def test_resnet_layout_is_untouched():
    from pairnet_amd import ResNet50Hip
    from pairnet_amd.backbone import _param_shapes
    from oracle.backbone import OracleResNet50
    for depth in (50, 101):
        want = [(k, tuple(v.shape)) for k, v in OracleResNet50(depth).state_dict().items()]
        assert [(k, tuple(s)) for k, s in _param_shapes(depth).items()] == want
    net = ResNet50Hip()
    assert net.groups == 1 and net.widths == (64, 128, 256, 512) and net.conv_algo == "winograd4"


def test_restated_backbone_fp32_stays_near_float64():
    """The seeded state is well conditioned: the restatement in fp32 stays within a tenth of the
    2e-4 (of each map's largest entry) the GPU test allows the kernels, and no map dies out."""
    P = GR.seeded_state(5, 50)
    img = torch.randn(1, 3, 64, 96, generator=GR.gen(6))
    want = GR.resnext(P, img, depth=50)
    got = GR.resnext(P, img, depth=50, dtype=torch.float32)
    assert [tuple(o.shape) for o in want] == [(1, 256, 16, 24), (1, 512, 8, 12), (1, 1024, 4, 6),
                                             (1, 2048, 2, 3)]
    for g, o in zip(got, want):
        assert float(o.abs().max()) > 1e-3
        assert float((g.double() - o).abs().max() / o.abs().max()) < 2e-5


@pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")
def test_reference_rnext_config_file_drops_in():
    """configs/deformable_detr/pairnet_rnext101_vg.py builds; its backbone section equals the
    restated one on every key, neck and head equal cross_r101_vg's; cross_r50_coco.py still fails."""
    from pairnet_amd import (ChannelMapper, CrossHeadBBox, ResNet50Hip, ResNeXtHip, build_detector,
                             cross_r101_vg, load_config, pairnet_rnext101_vg)
    cfg = load_config(os.path.join(ref_shim.REF_ROOT,
                                   "configs/deformable_detr/pairnet_rnext101_vg.py"))
    ours, r101 = pairnet_rnext101_vg().model, cross_r101_vg().model
    plain = lambda d: {k: (list(v) if isinstance(v, (tuple, list)) else v) for k, v in dict(d).items()}
    assert plain(cfg.model.backbone) == plain(ours.backbone)
    assert ours.backbone.type == "ResNeXt" and ours.backbone.with_cp is True
    assert plain(cfg.model.neck) == plain(ours.neck) == plain(r101.neck)
    ref_head, our_head = dict(cfg.model.bbox_head), dict(ours.bbox_head)
    assert our_head == dict(r101.bbox_head)
    assert {k: ref_head[k] for k in our_head} == our_head
    for model in (dict(cfg.model), dict(ours)):
        det = build_detector(model)
        assert type(det.backbone) is ResNeXtHip and isinstance(det.backbone, ResNet50Hip)
        assert det.backbone.depth == 101 and det.backbone.groups == 32
        assert det.backbone.widths == (256, 512, 1024, 2048) and det.out_indices == (1, 2, 3)
        assert isinstance(det.bbox_head, CrossHeadBBox) and isinstance(det.neck, ChannelMapper)
    bad = load_config(os.path.join(ref_shim.REF_ROOT, "configs/deformable_detr/cross_r50_coco.py"))
    with pytest.raises((ValueError, NotImplementedError, TypeError)):
        build_detector(dict(bad.model))


def test_restated_config_builds_without_the_reference():
    from pairnet_amd import ResNeXtHip, api, build_detector, cross_r101_vg, pairnet_rnext101_vg
    assert "ResNeXtHip" in api.__all__ and "pairnet_rnext101_vg" in api.__all__
    m = pairnet_rnext101_vg().model
    assert dict(m.backbone) == dict(type="ResNeXt", depth=101, groups=32, base_width=8,
                                    num_stages=4, out_indices=(1, 2, 3), frozen_stages=1,
                                    norm_cfg=dict(type="BN", requires_grad=False), norm_eval=True,
                                    style="pytorch", with_cp=True)
    assert dict(m.neck) == dict(cross_r101_vg().model.neck)
    bb = dict(m.backbone, depth=50)
    det = build_detector(dict(m, backbone=bb))
    assert type(det.backbone) is ResNeXtHip and det.backbone.depth == 50
    with pytest.raises(NotImplementedError, match="ResNeXt"):
        build_detector(dict(m, backbone=dict(type="RegNet")))


def test_unsupported_group_widths_and_keys_are_refused():
    from pairnet_amd import ResNeXtHip
    with pytest.raises(NotImplementedError, match=r"\[8, 16, 32, 64\]"):
        ResNeXtHip(101, 32, 4)                    # 32x4d: 4 channels per group in stage 1
    with pytest.raises(NotImplementedError, match=r"\[8, 16, 32, 64\]"):
        ResNeXtHip(50, 64, 4)
    with pytest.raises(NotImplementedError):
        ResNeXtHip(50, 32, 16)                    # 128 per group in stage 4
    with pytest.raises(NotImplementedError):
        ResNeXtHip(152, 32, 8)
    with pytest.raises(NotImplementedError, match="dcn"):
        ResNeXtHip(50, 32, 8, dcn=dict(type="DCN"))
    with pytest.raises(NotImplementedError):
        ResNeXtHip(50, 32, 8, style="caffe")
    ResNeXtHip(50, 32, 8, with_cp=True, norm_eval=True, frozen_stages=1)    # accepted, ignored


@pytest.fixture(scope="module")
def rnext50_cfg():
    from pairnet_amd import pairnet_rnext101_vg
    return dict(pairnet_rnext101_vg().model.backbone, depth=50, out_indices=(0, 1, 2, 3))


def test_trainers_refuse_a_resnext_backbone_before_any_device_use(rnext50_cfg):
    """No device here: a trainer that went on to tape the backbone would fail otherwise (or, as a
    subclass of the ResNet, pass the isinstance checks and fail in a backward kernel)."""
    from pairnet_amd import (BackboneGrad, PSGTr, ResNeXtHip, baseline_r50, pairnet_r50,
                             psgtr2_r50)
    for model, name in ((pairnet_r50(), "trainer"), (baseline_r50(), "full_trainer"),
                        (psgtr2_r50(), "triplet_trainer")):
        model = model.get("model", model)
        det = PSGTr(rnext50_cfg, model["bbox_head"], train_cfg=model.get("train_cfg"))
        assert type(det.backbone) is ResNeXtHip
        with pytest.raises(NotImplementedError, match="ResNeXt backbone: forward only"):
            getattr(det, name)(train_backbone=True)
    with pytest.raises(NotImplementedError, match="ResNeXt backbone: forward only"):
        BackboneGrad(det.backbone)


def test_boundary_carries_the_entry():
    from pairnet_amd import hip
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    assert re.search(r"\b%s\(" % ENTRY, header)
    assert "pairnet_rnext101_vg.py:9-21" in header and "restated from memory, unpinned" in header
    assert ENTRY in hip._SIGS and ENTRY in hip.EXPORTS
    assert len(hip._SIGS[ENTRY][1]) == 14
    assert not any(n.startswith("pn_tri_") and "grouped" in n for n in hip.EXPORTS)
    assert hip.ABI_VERSION == 34
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == 34
    assert callable(hip.conv3x3_grouped)
