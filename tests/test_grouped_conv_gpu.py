"""GPU: the grouped 3x3 convolution pn_conv2d_grouped_nhwc_f32 (csrc/grouped_conv.hip), the
ResNeXt backbone on it and the detector of pairnet_rnext101_vg(), under the contract of
tests/test_mm_kernels_gpu.py (its helpers are imported, not restated):

1. Exact cases.  Integer operands (x in [-8, 8], w in [-4, 4], a bias distinct per channel; every
   partial sum below 2^24: tests/test_resnext_refs.py) -> bit for bit the float64 statement of
   tests/grouped_conv_ref.py.  The instrument for group, halo, stride and tile-edge indexing.
2. Bounded cases.  Random operands on the same shapes: |got - ref| <= (L + a) 2^-24 mag + FLT_MIN
   on every element, L = 9 Cg + 1 (one fixed-order MFMA chain and the bias, counted from the
   kernel's source: grouped_conv_ref.chain, labnotes/r31.md), a = max(4, 2 x the ratio torch's own
   fp32 F.conv2d(groups=) reaches).  Nothing in the bound comes from the kernel under test.
3. Refusals.  PN_BAD_ARG surfaces as RuntimeError before anything is launched; the NaN-filled
   output stays NaN.
4. The backbone against its float64 restatement (2e-4 of each map's largest entry, the bound of the
   ResNet-101 test), hipGraph replay bit for bit the eager call.
5. The detector: `simple_test` equals the manual composition bit for bit; `box_train_step` moves
   the tail's parameters only.

Every kernel output is NaN-filled with a NaN fence behind it; every call runs twice and must give
equal bits."""
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import grouped_conv_ref as GR
from test_mm_kernels_gpu import _bound, _d, _equal, _fenced, _is_fence, _same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip as h
    h.lib()
    return h


def _run(hip, x, w, bias, c, relu):
    """The entry twice into fenced NaN outputs -> out [B][Ho][Wo][C]."""
    B, H, W, G, Cg, s = c
    Ho, Wo = GR.out_hw(H, W, s)
    xd, wd, bd = _d(x.contiguous()), _d(GR.pack_weight(w)), _d(bias)
    outs = []
    for _ in range(2):
        out, fence = _fenced(B, Ho, Wo, G * Cg)
        hip.conv3x3_grouped(xd, wd.view(G, Cg, 9 * Cg), bd, out, B, H, W, G, Cg, s, relu=relu)
        torch.cuda.synchronize()
        assert _is_fence(fence), "wrote past the output"
        outs.append(out)
    assert _same_bits(outs[0], outs[1]), "pn_conv2d_grouped_nhwc_f32 is not bitwise reproducible"
    return outs[0]


@pytest.mark.parametrize("ci", range(len(GR.CASES)))
def test_grouped_conv_exact(hip, ci):
    c = GR.CASES[ci]
    relu = GR.relu_of(ci)
    x, w, bias = GR.exact_operands(c, 300 + ci)
    ref, _ = GR.grouped_conv(x, w, bias, c[3], c[5], relu)
    _equal(_run(hip, x, w, bias, c, relu), ref, "%s relu %d" % (GR.case_name(c), relu))


@pytest.mark.parametrize("ci", range(len(GR.CASES)))
def test_grouped_conv_bounded(hip, ci):
    c = GR.CASES[ci]
    relu = GR.relu_of(ci)
    x, w, bias = GR.random_operands(c, 400 + ci)
    ref, mag = GR.grouped_conv(x, w, bias, c[3], c[5], relu)
    o32 = F.conv2d(x.permute(0, 3, 1, 2), w, bias, stride=c[5], padding=1,
                   groups=c[3]).permute(0, 2, 3, 1)
    o32 = F.relu(o32) if relu else o32
    got = _run(hip, x, w, bias, c, relu)
    _bound("grouped conv Cg %d" % c[4], "%s relu %d" % (GR.case_name(c), relu), got, ref, mag,
           GR.chain(c[4]), o32.contiguous())


BAD = [
    ("Cg 4", dict(Cg=4, G=16)), ("Cg 12", dict(Cg=12, G=4)), ("Cg 128", dict(Cg=128, G=1)),
    ("1x1", dict(kh=1, kw=1)), ("3x5", dict(kw=5)), ("5x3", dict(kh=5)),
    ("stride 0", dict(stride=0)), ("stride 3", dict(stride=3)), ("stride -1", dict(stride=-1)),
    ("relu-after-residual flag", dict(flags=128)), ("tile flag", dict(flags=4)),
    ("reserve flag", dict(flags=8 << 16)),
    ("G 0", dict(G=0)), ("B 0", dict(B=0)), ("H 0", dict(H=0)),
    # B H W C = 2^31 exactly, and well past it: the kernel indexes with int32
    ("int32 overflow", dict(B=2 ** 31 // (4 * 4 * 64))), ("int32 far", dict(B=2 ** 30)),
    ("misaligned input", dict(shift=1)), ("misaligned input by 8 bytes", dict(shift=2)),
    ("misaligned weights", dict(wshift=1)),               # (both are read as float4)
]


@pytest.mark.parametrize("bi", range(len(BAD)))
def test_grouped_conv_refusals(hip, bi):
    name, bad = BAD[bi]
    a = dict(B=1, H=4, W=4, G=8, Cg=8, stride=1, kh=3, kw=3, flags=0, shift=0, wshift=0)
    a.update(bad)
    n = 4 * 4 * 64
    x = torch.ones(n + 8, device=DEV)[a["shift"]:a["shift"] + n]
    nw = 64 * 9 * 128
    wg, bias = torch.ones(nw + 8, device=DEV)[a["wshift"]:a["wshift"] + nw], torch.ones(128, device=DEV)
    out, fence = _fenced(n)
    with pytest.raises(RuntimeError, match="argument contract"):
        hip.conv3x3_grouped(x, wg, bias, out, a["B"], a["H"], a["W"], a["G"], a["Cg"], a["stride"],
                            kh=a["kh"], kw=a["kw"], flags=a["flags"])
    torch.cuda.synchronize()
    assert _is_fence(out) and _is_fence(fence), name


def test_grouped_conv_accepts_what_the_refusals_vary(hip):
    """The refusal cases' base call is itself valid (ones: every inner output is 9 x 8 + 1)."""
    x, wg, bias = torch.ones(4 * 4 * 64, device=DEV), torch.ones(64 * 72, device=DEV), \
        torch.ones(64, device=DEV)
    out, fence = _fenced(1, 4, 4, 64)
    hip.conv3x3_grouped(x, wg, bias, out, 1, 4, 4, 8, 8, 1)
    torch.cuda.synchronize()
    assert _is_fence(fence) and float(out[0, 1, 1, 5]) == 73.0 and float(out[0, 0, 0, 63]) == 33.0


# ============================================================ the backbone
def _rel(got, want):
    want = want.double()
    return float((got.detach().cpu().double() - want).abs().max() / want.abs().max())


@pytest.fixture(scope="module")
def rnext101(built_lib):
    from pairnet_amd import ResNeXtHip
    P = GR.seeded_state(71, 101)
    net = ResNeXtHip(101, 32, 8)
    net.load_state_dict(P)
    return net.to(DEV), P


def _check_maps(got, want, B, H, W, chans):
    from pairnet_amd import ResNeXtHip
    assert len(got) == len(want) == 4
    for i, (g, o, (h, w)) in enumerate(zip(got, want, ResNeXtHip.feature_shapes(H, W))):
        assert tuple(g.shape) == tuple(o.shape) == (B, chans[i], h, w)
        assert g.is_contiguous(memory_format=torch.channels_last)
        assert float(o.abs().max()) > 1e-3
        e = _rel(g, o)
        print("C%d %s rel err %.2e (largest entry %.3g)" % (i + 2, tuple(o.shape), e,
                                                           float(o.abs().max())))
        assert e < 2e-4


@pytest.mark.parametrize("B,H,W", [(1, 75, 101), (2, 64, 96)])
def test_resnext101_matches_float64(rnext101, B, H, W):
    """(stage 4 is a 3 x 4 / 2 x 3 map behind a stride-2 grouped layer)"""
    net, P = rnext101
    img = torch.randn(B, 3, H, W, generator=GR.gen(72 + B))
    want = GR.resnext(P, img, 32, 8, 101)
    got = net(img.to(DEV))
    torch.cuda.synchronize()
    _check_maps(got, want, B, H, W, (256, 512, 1024, 2048))


def test_resnext101_graph_replay_equals_eager(rnext101):
    net, _ = rnext101
    img = torch.randn(2, 3, 64, 96, generator=GR.gen(79)).to(DEV)
    eager = [o.clone() for o in net(img, slot=1)]
    net.use_graphs, net.graph_after = True, 1
    try:
        net(img, slot=1)                                  # counted, eager
        for _ in range(2):                                # captured, then replayed again
            got = net(img, slot=1)
            torch.cuda.synchronize()
            assert net._plan(2, 64, 96, 1).graph is not None
            for g, e in zip(got, eager):
                assert _same_bits(g, e)
    finally:
        net.use_graphs = False


def test_resnext50_matches_float64(built_lib):
    from pairnet_amd import ResNeXtHip
    P = GR.seeded_state(81, 50)
    net = ResNeXtHip(50, 32, 8)
    net.load_state_dict(P)
    net.to(DEV)
    img = torch.randn(1, 3, 64, 96, generator=GR.gen(82))
    want = GR.resnext(P, img, 32, 8, 50)
    got = net(img.to(DEV))
    torch.cuda.synchronize()
    _check_maps(got, want, 1, 64, 96, (256, 512, 1024, 2048))


# ============================================================ the detector
# (the issue names a 96 x 128 image; its C3-C5 + stride-64 levels hold 256 tokens, fewer than the 300
# proposals of the config's head, which refuses them -- tests/test_bbox_train_gpu.py: 128 x 160 is
# the smallest image of that aspect the head accepts)
DH, DW = 128, 160


@pytest.fixture(scope="module")
def detector(rnext101):
    import pairnet_amd as P
    from oracle import seeded
    det = P.build_detector(P.pairnet_rnext101_vg().model)
    assert type(det.backbone) is P.ResNeXtHip
    det.backbone = rnext101[0]                            # the seeded backbone, packed once
    shapes = lambda m: OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())
    det.bbox_head.load_state_dict(seeded.seeded_state_dict(shapes(det.bbox_head), 3))
    det.neck.load_state_dict(seeded.seeded_state_dict(shapes(det.neck), 4))
    return det.to(DEV)


def _same(a, b, name):
    if a is None or b is None:
        assert a is None and b is None, name
    elif isinstance(a, torch.Tensor):
        assert _same_bits(a, b), name
    elif hasattr(a, "dtype"):                             # numpy
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), name
    elif isinstance(a, dict):
        assert set(a) == set(b), name
        for k in a:
            _same(a[k], b[k], "%s.%s" % (name, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), name
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (name, i))
    else:
        assert a == b, name


def test_detector_simple_test_is_the_manual_composition(detector):
    import pairnet_amd as P
    det = detector
    img = (torch.rand(1, 3, DH, DW, generator=GR.gen(91)) * 4.0 - 2.0).to(DEV)
    metas = [dict(batch_input_shape=(DH, DW), img_shape=(DH, DW, 3), scale_factor=[1.0] * 4)]
    out = det.simple_test(img, metas, rescale=True)
    assert len(out) == 1 and isinstance(out[0], P.Result)
    assert out[0].refine_bboxes.shape == (200, 5) and out[0].rel_dists.shape == (100, 51)
    assert out[0].masks is None and out[0].pan_results is None
    with torch.no_grad():
        c = det.backbone(img)
        assert [tuple(t.shape[1:]) for t in c] == [(256, 32, 40), (512, 16, 20), (1024, 8, 10),
                                                   (2048, 4, 5)]
        feats = det.neck(tuple(c[i] for i in (1, 2, 3)))
        trip = det.bbox_head.simple_test(feats, metas, rescale=True)
        want = P.triplet2Result(trip[0], det.bbox_head.use_mask)
    for k in P.Result.FIELDS:
        _same(getattr(out[0], k), getattr(want, k), k)


def test_detector_box_train_step_moves_the_tail_only(detector):
    import bbox_loss_ref as BR
    import pairnet_amd as P
    det = detector
    B = 2
    img = (torch.rand(B, 3, DH, DW, generator=GR.gen(92)) * 4.0 - 2.0).to(DEV)
    metas = [dict(batch_input_shape=(DH, DW), img_shape=(DH, DW, 3), scale_factor=[1.0] * 4)] * B
    case = BR.make_case(seed=11, G=(4, 6), T=(3, 7), num_classes=150, num_relations=50,
                        batch_shape=(DH, DW), planted=False)
    gt = (case["gt_rels"], case["gt_bboxes"], case["gt_labels"])
    for name in ("trainer", "full_trainer", "triplet_trainer"):
        with pytest.raises(NotImplementedError):
            getattr(det, name)(train_backbone=True)
    vals = det.val_box_losses(img, metas, *gt)
    assert set(vals) == {"loss_r_cls", "loss_sub_cls", "loss_obj_cls", "loss_match"}
    tr = det.box_trainer()
    assert isinstance(tr, P.BBoxTrainer)
    version = det.backbone._weights_version()
    p0 = tr.flat_p.clone()
    head_sd = det.bbox_head.state_dict()
    frozen = {k: v.clone() for k, v in det.bbox_head.w.items() if k in head_sd and k not in tr.layout}
    bbw = {k: v.clone() for k, v in det.backbone.w.items()}
    neckw = {k: v.clone() for k, v in det.neck.w.items()}
    out = det.box_train_step(img, metas, *gt)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v)) for v in out.values()) and float(out["grad_norm"]) > 0
    assert not torch.equal(p0, tr.flat_p)
    for n, (o, shape, k) in tr.layout.items():
        assert float((tr.flat_p[o:o + k] - p0[o:o + k]).abs().max()) > 0, n
    assert frozen and all(_same_bits(v, det.bbox_head.w[k]) for k, v in frozen.items())
    assert det.backbone._weights_version() == version
    assert set(bbw) == set(det.backbone.w) and all(_same_bits(v, det.backbone.w[k])
                                                   for k, v in bbw.items())
    assert all(_same_bits(v, det.neck.w[k]) for k, v in neckw.items())
