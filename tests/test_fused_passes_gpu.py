"""GPU: passes folded into neighbouring kernels give the bits of the launch sequence they replace.

`pn_bottleneck_proj_f32` (csrc/gemm.hip, k_gemm_proj): projection shortcut + conv3 of a stage's
first bottleneck in one launch, against the shortcut launch into `idt` followed by conv3 with
`idt` as its residual -- `torch.equal`, at the four stage geometries of an 800 x 1333 image and
at ragged ones (rows not a multiple of 64, odd sides, two images).  Where the library's split-K /
skinny rules would change the summation order of either launch it issues the two launches itself;
the cases say which form they expect, and the `idt` workspace (untouched by the one-launch form)
shows which one ran.

`pn_mask_stencil_gather_gemm_f32` (k_gemm_stencil_gather): a decoder layer's attention-mask bits
with the stencil rows read in place from the mask feature, against pn_bilinear_stencil_rows_f32
followed by pn_mask_stencil_gemm_f32 -- equal bits and row flags at the three levels of an
800 x 1333 image and at odd / ragged maps.

`pn_groupnorm_upadd_nhwc_f32` (csrc/norm.hip, k_gn_apply_up): the lateral GroupNorm and the
top-down bilinear upsample-add in one pass, `torch.equal` to pn_groupnorm_nhwc_f32 followed by the
accumulating pn_bilinear_nhwc_f32.

Then the backbone and the whole detector with every switch on against every switch off, and the
switches' place in the plan key / graph configuration."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def R(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _two_launches(hip, x, wsc, bsc, t2, w3, b3, idt, out, B, H, W, cin, planes, stride, scratch):
    cout = w3.shape[0]
    if stride == 1:
        hip.linear(x.view(-1, cin), wsc, bsc, idt.view(-1, cout), scratch=scratch)
    else:
        hip.conv2d_ex(x, wsc, bsc, None, idt, B, H, W, cin, cout, 1, 1, stride, 0, scratch=scratch)
    hip.linear(t2.view(-1, planes), w3, b3, out.view(-1, cout), res=idt.view(-1, cout),
               relu_after=True, scratch=scratch)


# (B, H, W, Cin, planes, stride, one launch expected)
PROJ_CASES = [
    # the first blocks of the four stages at 800 x 1333 (1056-4176 and 544 tiles: never split)
    (1, 200, 334, 64, 64, 1, True), (1, 200, 334, 256, 128, 2, True),
    (1, 100, 167, 512, 256, 2, True), (1, 50, 84, 1024, 512, 2, True),
    # ragged: 3233 / 1794 / 896 / 621 rows per image, two images, odd sides
    (2, 61, 53, 64, 64, 1, True), (2, 77, 91, 256, 128, 2, True),
    (2, 55, 63, 512, 256, 2, True), (2, 45, 53, 1024, 512, 2, True),
    # the rules take the two-launch form: skinny kernel (few tiles), split-K shortcut (K = 1024
    # over 2 x 8 x 32 = 512 tiles)
    (2, 13, 17, 64, 64, 1, False), (1, 30, 41, 256, 128, 2, False),
    (2, 41, 45, 1024, 512, 2, False),
]


@pytest.mark.parametrize("B,H,W,cin,planes,stride,one_launch", PROJ_CASES)
def test_bottleneck_proj_equals_the_two_launches(B, H, W, cin, planes, stride, one_launch):
    from pairnet_amd import hip
    cout = planes * 4
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = R(B, H, W, cin, seed=1).to(DEV)
    t2 = R(B, Ho, Wo, planes, seed=2).relu_().to(DEV)
    wsc, bsc = R(cout, cin, seed=3, scale=cin ** -0.5).to(DEV), R(cout, seed=4).to(DEV)
    w3, b3 = R(cout, planes, seed=5, scale=planes ** -0.5).to(DEV), R(cout, seed=6).to(DEV)
    scratch = torch.empty(8 * 1024 * 1024, device=DEV)
    idt = torch.empty(B, Ho, Wo, cout, device=DEV)
    want = torch.empty(B, Ho, Wo, cout, device=DEV)
    _two_launches(hip, x, wsc, bsc, t2, w3, b3, idt, want, B, H, W, cin, planes, stride, scratch)
    got = torch.full_like(want, float("nan"))
    work = torch.full_like(idt, -7.0)
    hip.bottleneck_proj(x, wsc, bsc, t2, w3, b3, work, got, B, H, W, cin, planes, stride,
                        scratch=scratch)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert bool((work == -7.0).all()) == one_launch
    # and it is the bottleneck's output, not just the same bits: fp64 on the host
    xs = x[:, ::stride, ::stride].reshape(-1, cin).double().cpu()
    ref = (t2.view(-1, planes).double().cpu() @ w3.double().cpu().T + b3.double().cpu()
           + xs @ wsc.double().cpu().T + bsc.double().cpu()).relu()
    err = float((got.view(-1, cout).double().cpu() - ref).abs().max() / ref.abs().max())
    print("rel err vs fp64 %.2e" % err)
    assert err < 2e-5


def test_bottleneck_proj_refuses_bad_arguments():
    from pairnet_amd import hip
    lib = hip.lib()
    a = torch.zeros(64 * 64, device=DEV).data_ptr()
    assert lib.pn_bottleneck_proj_f32(None, a, a, a, a, a, a, a, 1, 8, 8, 64, 64, 256, 1, 0, None, 0,
                                      None) == -1
    assert lib.pn_bottleneck_proj_f32(a, a, a, a, a, a, a, a, 1, 8, 8, 48, 64, 256, 1, 0, None, 0,
                                      None) == -1       # Cin % 32
    assert lib.pn_bottleneck_proj_f32(a, a, a, a, a, a, a, a, 1, 8, 8, 64, 64, 256, 0, 0, None, 0,
                                      None) == -1       # stride


# (hi, wi) the mask-feature map, (ho, wo) the level's map
@pytest.mark.parametrize("B,Q,hi,wi,ho,wo", [
    (1, 100, 200, 334, 25, 42), (1, 100, 200, 334, 50, 84), (1, 100, 200, 334, 100, 167),
    (2, 100, 51, 37, 7, 5), (2, 37, 24, 32, 12, 16), (2, 200, 29, 43, 15, 22), (1, 100, 9, 11, 9, 11)])
def test_stencil_gather_gemm_equals_rows_then_gemm(B, Q, hi, wi, ho, wo):
    from pairnet_amd import hip
    C = 256
    g = torch.Generator().manual_seed(hi * wi + ho)
    mf = torch.randn(B, hi * wi, C, generator=g).to(DEV)
    me = torch.randn(B * Q, C, generator=g).to(DEV)
    me[min(3, B * Q - 1)] = -1.0       # one row that masks most keys of a non-negative feature
    n = ho * wo
    nw = (n + 31) // 32
    for feat in (mf, mf.abs()):        # (the second: row 3 has every key masked, rowall = 1)
        rows = torch.empty(B, 4 * n, C, device=DEV)
        hip.bilinear_stencil_rows(feat, rows, B, hi, wi, ho, wo, C, hi * wi * C, 4 * n * C)
        bits_w = torch.full((B * Q * nw,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
        all_w = torch.full((B * Q,), 7, dtype=torch.int32, device=DEV)
        hip.mask_stencil_gemm(me, rows, bits_w, all_w, B, Q, hi, wi, ho, wo, K=C)
        bits_g = torch.full_like(bits_w, 0x33333333)
        all_g = torch.full_like(all_w, 9)
        hip.mask_stencil_gather_gemm(me, feat, bits_g, all_g, B, Q, hi, wi, ho, wo, K=C)
        torch.cuda.synchronize()
        assert torch.equal(bits_g, bits_w) and torch.equal(all_g, all_w)
    assert int(all_g[min(3, B * Q - 1)]) == 1 and int(all_g.sum()) < B * Q


def test_stencil_gather_gemm_refuses_bad_arguments():
    from pairnet_amd import hip
    lib = hip.lib()
    a = torch.zeros(64 * 256, device=DEV).data_ptr()
    ok = (a, 256, 0, a, 256, 0, a, a, 1, 8, 64, 256, 8, 8, 8, 8, 0, None)
    bad = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    assert lib.pn_mask_stencil_gather_gemm_f32(*bad(3, None)) == -1
    assert lib.pn_mask_stencil_gather_gemm_f32(*bad(10, 63)) == -1      # Nk != ho * wo
    assert lib.pn_mask_stencil_gather_gemm_f32(*bad(11, 48)) == -1      # K % 32
    assert lib.pn_mask_stencil_gather_gemm_f32(*bad(4, 254)) == -1      # ld % 4


# (B, H, W) the stride-4 map, (hc, wc) the coarse memory; the memories of all levels share one
# buffer (batch stride > hc * wc * 256), as in the head
@pytest.mark.parametrize("B,H,W,hc,wc", [(1, 200, 334, 100, 167), (2, 51, 37, 26, 19),
                                         (2, 24, 32, 12, 16), (1, 33, 29, 17, 15), (2, 9, 300, 5, 150)])
def test_groupnorm_upadd_equals_groupnorm_then_accumulate(B, H, W, hc, wc):
    from pairnet_amd import hip
    HW, G = H * W, 32
    x = (R(B, HW, 256, seed=11) * 3.0 + 0.5).to(DEV)
    gamma, beta = R(256, seed=12).to(DEV), R(256, seed=13).to(DEV)
    mem = R(B, hc * wc + 77, 256, seed=14).to(DEV)
    coarse = mem[:, 77:]
    part = torch.empty(B * hip.lib().pn_groupnorm_nblk(HW) * G * 2, dtype=torch.float64, device=DEV)
    want = torch.empty(B, HW, 256, device=DEV)
    hip.groupnorm_nhwc(x, gamma, beta, want, part, B, HW, G, False, HW * 256, HW * 256)
    hip.bilinear_nhwc(coarse, want, B, hc, wc, H, W, 256, True, mem.stride(0), HW * 256)
    got = torch.full_like(want, float("nan"))
    part.fill_(float("nan"))
    hip.groupnorm_upadd_nhwc(x, gamma, beta, got, part, coarse, B, H, W, hc, wc, G, HW * 256,
                             HW * 256, mem.stride(0))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # and it is GroupNorm + F.interpolate, not just the same bits
    import torch.nn.functional as F
    xc = x.cpu().double().view(B, H, W, 256).permute(0, 3, 1, 2)
    up = F.interpolate(coarse.cpu().double().reshape(B, hc, wc, 256).permute(0, 3, 1, 2), size=(H, W),
                       mode="bilinear", align_corners=False)
    ref = F.group_norm(xc, G, gamma.cpu().double(), beta.cpu().double(), 1e-5) + up
    err = float((got.cpu().double().view(B, H, W, 256).permute(0, 3, 1, 2) - ref).abs().max())
    print("max abs err vs fp64 %.2e" % err)
    assert err < 2e-5 * float(ref.abs().max())


def _net(fused):
    from oracle.backbone import seeded_backbone_state
    from pairnet_amd import ResNet50Hip
    net = ResNet50Hip()
    net.load_state_dict(seeded_backbone_state(31))
    net.fuse_proj_shortcut = fused
    return net.to(DEV)


@pytest.mark.parametrize("B,H,W", [(1, 800, 1333), (2, 75, 101)])
def test_backbone_features_equal_with_and_without_the_fused_shortcut(B, H, W):
    img = R(B, 3, H, W, seed=8).to(DEV)
    want = [f.clone() for f in _net(False)(img)]
    got = _net(True)(img)
    torch.cuda.synchronize()
    for i, (g, o) in enumerate(zip(got, want)):
        assert torch.equal(g, o), "C%d" % (i + 2)


@pytest.mark.parametrize("H,W", [(800, 1333), (203, 149)])
def test_detector_results_equal_with_all_switches_on_and_off(H, W):
    """image -> backbone -> head -> Result: every field, all switches on against all off."""
    from helpers import oracle_head
    from oracle import seeded
    from oracle.backbone import seeded_backbone_state
    from pairnet_amd import build_detector, pairnet_r50
    from pairnet_amd.detector import Result
    _, sd, _ = oracle_head(1234)
    det = build_detector(pairnet_r50())
    det.backbone.load_state_dict(seeded_backbone_state(31))
    det.bbox_head.load_state_dict(sd)
    det.to(DEV)
    img = seeded.uniform(np.random.default_rng(H * 1000 + W), (1, 3, H, W), -2.0, 2.0).to(DEV)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4)]
    res = {}
    for fused in (False, True):
        det.backbone.fuse_proj_shortcut = fused
        det.bbox_head.gather_mask_stencil = det.bbox_head.fuse_lateral_upadd = fused
        r = det.simple_test(img, metas)[0]
        res[fused] = {}
        for k in Result.FIELDS:
            v = getattr(r, k)
            for kk, vv in (v.items() if isinstance(v, dict) else [("", v)]):   # formatted_masks
                if vv is not None:
                    res[fused][k + "." + kk] = np.array(vv, copy=True)
    assert res[True].keys() == res[False].keys() and len(res[True]) >= 8
    for k in res[True]:
        assert res[True][k].dtype != object, k
        assert np.array_equal(res[True][k], res[False][k]), k


def test_flipping_the_switch_after_a_capture_replans():
    """The plan key carries the switch: a graph captured with it on is not replayed once it is
    off (and the other way round), each setting keeps its own plan, and both give the same
    features."""
    net = _net(True)
    net.use_graphs = True
    img = R(1, 3, 96, 128, seed=9).to(DEV)
    for _ in range(3):
        torch.cuda.synchronize()            # (graphs are captured at quiet points only)
        on = [f.clone() for f in net(img)]
    torch.cuda.synchronize()
    pl_on = net._plan(1, 96, 128)
    assert pl_on.graph is not None
    net.fuse_proj_shortcut = False
    pl_off = net._plan(1, 96, 128)
    assert pl_off is not pl_on and pl_off.graph is None
    for _ in range(3):
        torch.cuda.synchronize()
        off = [f.clone() for f in net(img)]
    torch.cuda.synchronize()
    assert net._plan(1, 96, 128).graph is not None
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    net.fuse_proj_shortcut = True
    assert net._plan(1, 96, 128) is pl_on


@pytest.mark.parametrize("switch,pos", [("gather_mask_stencil", -2), ("fuse_lateral_upadd", -1)])
def test_head_graph_configuration_carries_the_switches(switch, pos):
    """Stage graphs bake the launch sequence in: after a capture, flipping a switch
    drops the captured stages (they are captured again for the new sequence) and the results
    stay the same."""
    from helpers import head_cfg, oracle_head
    from pairnet_amd import CrossHead2
    _, sd, _ = oracle_head(1234)
    head = CrossHead2(**head_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    head.use_graphs = True
    setattr(head, switch, True)
    H, W = 96, 128
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(1, c, H // s, W // s, generator=g).to(DEV)
             for c, s in zip((256, 512, 1024, 2048), (4, 8, 16, 32))]
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4)]

    def run():
        for _ in range(3):
            torch.cuda.synchronize()
            r = head.simple_test_bboxes(feats, metas)[0]
        torch.cuda.synchronize()
        return [t.clone() for t in r if torch.is_tensor(t)]

    on = run()
    pl = head._last_plan
    cfg_on = pl.graph_cfg
    graph_on = pl.graph_b
    assert cfg_on[pos] is True and graph_on is not None and pl.graph_a is not None
    setattr(head, switch, False)
    off = run()
    pl = head._last_plan
    assert pl.graph_cfg != cfg_on and pl.graph_cfg[pos] is False
    assert pl.graph_b is not None and pl.graph_b is not graph_on
    assert len(on) == len(off) and len(on) >= 4
    for a, b in zip(on, off):
        assert torch.equal(a, b)
