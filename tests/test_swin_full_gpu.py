"""GPU: a Swin backbone whose every stage trains (configs/deformable_detr/cross_swinb_vg.py:202-226,
frozen_stages=-1) -- `pn_patch_merge_ln_bwd_f32`, the patch-embedding backward, the tape over all
stages (grad.py SwinStagesGrad) and its training step (TailTrainer) -- against the float64 statements
of tests/swin_full_ref.py and float64 autograd through oracle/swin.py.

Tiny backbone (embed 32, depths 2-2-2-2, window 4), B = 2, image 3 x 50 x 70: maps 13x18, 7x9, 4x5,
2x3 -- a merge with odd H, one with both sides odd, one with odd W; every map needs window padding.

Bounds.  Kernels: 1e-4 of each tensor's largest entry against float64 (tests/test_swin_grad_gpu.py).
Whole tape: per tensor the larger of 1e-4 and 4 x the error of the SAME oracle's autograd run in
fp32 against its float64 run (the chain is four stages deep; the factor 4 covers the different
summation orders of the GEMMs and column sums)."""
import numpy as np
import pytest
import torch

from oracle.swin import OracleSwin, seeded_swin_state
from swin_full_ref import (BATCH, DIMS, IMG_H, IMG_W, frozen, oracle_backward, patch_embed_bwd,
                           patch_merge_ln_bwd, to_unfold)
from test_grad_gpu import _compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NBLK = sum(DIMS["depths"])
DROP_PATH = 0.3


def R(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 32), (2, 13, 18, 32), (2, 7, 9, 64), (1, 1, 5, 128),
                                     (1, 4, 6, 768)])
def test_patch_merge_ln_bwd_matches_float64(B, H, W, C):
    from pairnet_amd import hip
    rows = B * ((H + 1) // 2) * ((W + 1) // 2)
    x = R(B, H, W, C, seed=1, scale=2.0) + 0.3
    dy, gamma = R(rows, 4 * C, seed=2), R(4 * C, seed=3, scale=0.3) + 1.0     # neighbour-major
    addend = R(B * H * W, C, seed=4)
    dx_ref, dg_ref, db_ref = patch_merge_ln_bwd(dy, x, gamma, 1e-5, B, H, W, C)
    nblk = hip.patch_merge_ln_bwd_nblocks(B, H, W)
    assert nblk == min(-(-rows // 4), 512)
    xd, dyd, gd = x.view(-1, C).to(DEV), dy.to(DEV), gamma.to(DEV)
    dx, part = _nan(B * H * W, C), _nan(nblk, 8 * C)
    hip.patch_merge_ln_bwd(dyd, xd, gd, dx, part, B, H, W, C)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx).all())          # every dx row is written
    assert bool(torch.isfinite(part).all())
    report = []
    _compare("dx", dx.view(B, H, W, C), dx_ref, report)
    gb = torch.empty(8 * C, device=DEV)
    hip.colsum(part, gb)
    _compare("d gamma (kernel order)", gb[:4 * C], dg_ref, report)
    _compare("d beta (kernel order)", gb[4 * C:], db_ref, report)
    _compare("d gamma (nn.Unfold order)", to_unfold(gb[:4 * C], C), to_unfold(dg_ref, C), report)
    _compare("d beta (nn.Unfold order)", to_unfold(gb[4 * C:], C), to_unfold(db_ref, C), report)
    for name, scale, err in report:
        print("%-28s max |ref| %.3e  error %.2e (%.1e relative)" % (name, scale, err, err / scale))
    # accumulate = a plain launch + the addend, bit for bit
    acc, part2 = addend.to(DEV), _nan(nblk, 8 * C)
    hip.patch_merge_ln_bwd(dyd, xd, gd, acc, part2, B, H, W, C, accumulate=True)
    assert torch.equal(acc, addend.to(DEV) + dx)
    # two launches: equal bits
    dx3, part3 = _nan(B * H * W, C), _nan(nblk, 8 * C)
    hip.patch_merge_ln_bwd(dyd, xd, gd, dx3, part3, B, H, W, C)
    assert torch.equal(dx3, dx) and torch.equal(part3, part) and torch.equal(part2, part)
    # refusals: a non-zero code, the fenced outputs untouched
    fdx, fpart = _nan(B * H * W, C), _nan(nblk, 8 * C)
    for b, h, w, c in ((B, H, W, C + 2), (B, H, W, 772), (B, 0, W, C), (B, H, 0, C), (0, H, W, C)):
        code = hip.lib().pn_patch_merge_ln_bwd_f32(hip._ptr(dyd), hip._ptr(xd), hip._ptr(gd),
                                                   hip._ptr(fdx), hip._ptr(fpart), nblk, b, h, w, c,
                                                   1e-5, 0, hip._stream())
        assert code != 0, (b, h, w, c)
    torch.cuda.synchronize()
    assert bool(torch.isnan(fdx).all()) and bool(torch.isnan(fpart).all())


# ---------------------------------------------------------------- the tape
@pytest.fixture(scope="module")
def oracle():
    m = OracleSwin(**DIMS)
    m.load_state_dict(seeded_swin_state(m, 7))
    return m


@pytest.fixture(scope="module")
def tapes(oracle):
    from pairnet_amd import SwinStagesGrad, SwinTransformerHip
    out = {}
    for f in (-1, 1):
        swin = SwinTransformerHip(frozen_stages=f, drop_path_rate=DROP_PATH, **DIMS)
        swin.load_state_dict(oracle.state_dict())
        swin.to(DEV)
        out[f] = (swin, SwinStagesGrad(swin))
    return out


def _image():
    return R(BATCH, 3, IMG_H, IMG_W, seed=12)


def _map_grads(seed=20):
    shapes = [(13, 18, 32), (7, 9, 64), (4, 5, 128), (2, 3, 256)]
    return [R(BATCH, h, w, c, seed=seed + i) for i, (h, w, c) in enumerate(shapes)]


def _keep():
    """A fixed mix of 0 and 1 / (1 - p) at mmdet's rates linspace(0, drop_path_rate, sum(depths))."""
    rates = torch.linspace(0, DROP_PATH, NBLK, dtype=torch.float64).float()
    keep = (1.0 / (1.0 - rates)).view(-1, 1, 1).expand(NBLK, 2, BATCH).clone()
    for j, br, b in ((1, 0, 1), (2, 1, 0), (3, 1, 1), (4, 0, 0), (5, 1, 0), (6, 0, 1), (7, 1, 1)):
        keep[j, br, b] = 0.0
    return keep


def test_patch_embed_bwd_matches_autograd(oracle, tapes):
    swin, tape = tapes[-1]
    img = _image()
    tape.forward(img.to(DEV))
    C = DIMS["embed_dims"]
    G = R(BATCH * 13 * 18, C, seed=30)
    grads = tape._zero_grads()
    tape._patch_embed_bwd(G.to(DEV), grads)
    pe = oracle.patch_embed
    ref = patch_embed_bwd(img, G, pe.projection.weight.detach(), pe.projection.bias.detach(),
                          pe.norm.weight.detach(), pe.norm.eps)
    # the statement itself is autograd's (host test); once more directly, through the module
    m = __import__("copy").deepcopy(pe).double()
    tok, _ = m(img.double())
    (tok.reshape(-1, C) * G.double()).sum().backward()
    report = []
    for n, p in m.named_parameters():
        assert tuple(grads["patch_embed." + n].shape) == tuple(p.shape)        # [C][3][4][4]
        _compare("patch_embed." + n, grads["patch_embed." + n], p.grad, report)
        _compare("patch_embed." + n + " (statement)", grads["patch_embed." + n], ref[n], report)


@pytest.mark.parametrize("f,with_keep,with_c2", [(-1, False, False), (-1, True, False),
                                                 (-1, False, True), (1, False, False),
                                                 (1, True, False)])
def test_swin_stages_tape_matches_autograd(oracle, tapes, f, with_keep, with_c2):
    swin, tape = tapes[f]
    img, G = _image(), _map_grads()
    keep = _keep() if with_keep else None
    d_maps = [G[0] if with_c2 else None, G[1], G[2], G[3]]
    outs64, ref = oracle_backward(oracle, img, d_maps, f, keep, torch.float64)
    _, ref32 = oracle_backward(oracle, img, d_maps, f, keep, torch.float32)
    maps = tape.forward(img.to(DEV), keep=keep)
    report = []
    for i, (m, o) in enumerate(zip(maps, outs64)):
        _compare("C%d" % (i + 2), m, o, report)
    nchw = lambda g: None if g is None else g.to(DEV).permute(0, 3, 1, 2)
    grads = tape.backward(nchw(d_maps[1]), nchw(d_maps[2]), nchw(d_maps[3]), d_c2=nchw(d_maps[0]))
    torch.cuda.synchronize()
    # frozen modules have no entry; everything autograd reaches has one
    assert not any(frozen(n, f) for n in grads)
    assert set(ref) <= set(grads)
    assert set(grads) - set(ref) <= {"norm0.weight", "norm0.bias"}
    print("%-52s %10s %12s %12s" % ("tensor", "max |g|", "fp32 oracle", "GPU tape"))
    bad = []
    for n in grads:
        got = grads[n].cpu().double()
        if n not in ref:                           # norm0 without d_c2: no gradient
            assert not with_c2 and float(got.abs().max()) == 0.0, n
            continue
        assert tuple(got.shape) == tuple(ref[n].shape), n
        scale = float(ref[n].abs().max())
        e32 = float((ref32[n].double() - ref[n]).abs().max()) / scale
        egpu = float((got - ref[n]).abs().max()) / scale
        print("%-52s %10.3e %12.2e %12.2e" % (n, scale, e32, egpu))
        if not egpu <= max(1e-4, 4.0 * e32):
            bad.append((n, egpu, e32))
    assert not bad, bad
    # bitwise reproducible: a second backward of the same tape
    first = tape.flat_grad.clone()
    tape.backward(nchw(d_maps[1]), nchw(d_maps[2]), nchw(d_maps[3]), d_c2=nchw(d_maps[0]))
    assert torch.equal(tape.flat_grad, first)


def test_swin_stages_maps_match_inference(tapes):
    swin, tape = tapes[-1]
    img = _image().to(DEV)
    swin.gemm_arithmetic = "fp32"
    try:
        feats = [f.clone() for f in swin(img)]
    finally:
        swin.gemm_arithmetic = "bf16x3"
    maps = tape.forward(img)
    for i in (1, 2, 3):                            # C3, C4, C5
        ref = feats[i].permute(0, 2, 3, 1)
        assert float((maps[i] - ref).abs().max()) <= 2e-4 * float(ref.abs().max()), i


# ---------------------------------------------------------------- the training step
def _tiny_detector(f):
    from pairnet_amd import build_detector, pairnet_swin
    from pairnet_amd.config import pairnet_head_cfg
    cfg = pairnet_swin("B")
    cfg["backbone"].update(embed_dims=DIMS["embed_dims"], depths=list(DIMS["depths"]),
                           num_heads=list(DIMS["num_heads"]), window_size=DIMS["window_size"],
                           frozen_stages=f, drop_path_rate=DROP_PATH)
    head = pairnet_head_cfg(in_channels=[32, 64, 128, 256])
    head.pop("mapper")
    head["strides"] = [4, 8, 16, 32]
    cfg["bbox_head"] = head
    det = build_detector(cfg)
    det.bbox_head.init_weights(seed=4)
    det.to(DEV)
    return cfg, det


def _batch():
    g = torch.Generator().manual_seed(9)
    H, W = IMG_H, IMG_W
    img = torch.randn(BATCH, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4, batch_input_shape=(H, W))
             for _ in range(BATCH)]
    gt_labels = [torch.tensor([3, 17, 90, 120]), torch.tensor([5, 60, 101])]
    gt_masks = [(torch.rand(len(l), H, W, generator=g) > 0.6).numpy() for l in gt_labels]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 3, 17], [1, 0, 56]]), torch.tensor([[0, 2, 9], [1, 0, 30]])]
    return img, metas, gt_rels, gt_labels, gt_masks


def test_swin_full_train_step_from_the_image():
    from pairnet_amd import SwinBackboneGrad, SwinStagesGrad, SwinTransformerHip
    cfg, det = _tiny_detector(-1)
    img, metas, gt_rels, gt_labels, gt_masks = _batch()
    bb0 = {k: v.clone() for k, v in det.backbone.state_dict().items()}
    lr = 1e-3
    tr = det.trainer(train_backbone=True, lr=lr, decay_mult={"backbone.": 0.0})
    assert tr.swin and type(tr.bb_tape) is SwinStagesGrad
    lrs, wds = tr.seg_lr.cpu(), tr.seg_wd.cpu()
    for i, n in enumerate(tr.layout):
        if n.startswith("backbone.norm0."):
            assert float(lrs[i]) == 0.0 and float(wds[i]) == 0.0, n
        elif n.startswith("backbone."):
            assert abs(float(lrs[i]) - 0.01) < 1e-9 and float(wds[i]) == 0.0, n
    p0 = tr.flat_p.clone()
    out = det.train_step(img, metas, gt_rels, None, gt_labels, gt_masks)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in out.values()) and float(out["grad_norm"]) > 0
    # the first update of every trained tensor = torch's AdamW + clip on the tape's own gradients
    gflat = tr.flat_grad.cpu().double()
    coef = min(1.0, tr.max_norm / (float(gflat.norm()) + 1e-6))
    worst = 0.0
    for n, v in tr.params.items():
        o, shape, k = tr.layout[n]
        i = list(tr.layout).index(n)
        p = p0[o:o + k].cpu().double().requires_grad_()
        opt = torch.optim.AdamW([p], lr=lr * float(lrs[i]), weight_decay=tr.wd * float(wds[i]),
                                betas=tr.betas, eps=tr.eps)
        p.grad = gflat[o:o + k] * coef
        opt.step()
        worst = max(worst, float((v.reshape(-1).cpu().double() - p.detach()).abs().max()))
    print("first AdamW update: worst |difference| vs torch %.2e (lr %.0e)" % (worst, lr))
    assert worst < 2e-2 * lr
    tr.write_back()
    bb1 = det.backbone.state_dict()
    moved = {k for k in bb1 if not torch.equal(bb1[k].cpu(), bb0[k].cpu())}
    names = {n for _, ns in tr.bb_tape.param_groups(det.backbone) for n in ns}
    assert moved <= names - {"norm0.weight", "norm0.bias"}
    assert {"patch_embed.projection.weight", "patch_embed.norm.weight",
            "stages.0.downsample.norm.weight", "stages.0.downsample.reduction.weight",
            "stages.1.downsample.reduction.weight", "stages.2.downsample.norm.bias",
            "stages.0.blocks.0.attn.w_msa.relative_position_bias_table",
            "stages.2.blocks.1.ffn.layers.1.weight", "norm1.weight", "norm3.bias"} <= moved
    for k in ("norm0.weight", "norm0.bias"):       # bitwise unchanged
        assert torch.equal(bb1[k].cpu(), bb0[k].cpu())
    # a fresh backbone from the written-back state dict computes bit for bit what the trained one
    # computes: every derived pack (.s3 splits, transposed bias tables, the neighbour-major
    # patch-merging norm / reduction, the padded patch-embedding weight) was refreshed in place
    bcfg = {k: v for k, v in cfg["backbone"].items() if k != "type"}
    fresh = SwinTransformerHip(**bcfg)
    fresh.load_state_dict(bb1)
    fresh.to(DEV)
    for mode in ("bf16x3", "fp32"):
        det.backbone.gemm_arithmetic = fresh.gemm_arithmetic = mode
        a = [f.clone() for f in det.backbone(img)]
        b = [f.clone() for f in fresh(img)]
        assert all(torch.equal(x, y) for x, y in zip(a, b)), mode
    det.backbone.gemm_arithmetic = "bf16x3"

    # frozen_stages=1: patch_embed, stage 0 with its downsample and norm0 stay where they were
    cfg1, det1 = _tiny_detector(1)
    s0 = {k: v.clone() for k, v in det1.backbone.state_dict().items()}
    tr1 = det1.trainer(train_backbone=True, lr=lr, decay_mult={"backbone.": 0.0})
    assert type(tr1.bb_tape) is SwinStagesGrad
    det1.train_step(img, metas, gt_rels, None, gt_labels, gt_masks)
    tr1.write_back()
    s1 = det1.backbone.state_dict()
    moved1 = {k for k in s1 if not torch.equal(s1[k].cpu(), s0[k].cpu())}
    assert moved1 and not any(k.startswith(("patch_embed.", "stages.0.", "norm0.")) for k in moved1)
    assert "stages.1.downsample.reduction.weight" in moved1 and "norm1.weight" in moved1

    # frozen_stages=3 still builds the last-stage tape
    cfg3, det3 = _tiny_detector(3)
    assert type(det3.trainer(train_backbone=True).bb_tape) is SwinBackboneGrad

    # the optimizer block's backbone key supplies decay_mult when the config carries one
    from pairnet_amd import build_detector
    cfg_o = dict(cfg, optimizer=dict(paramwise_cfg=dict(custom_keys=dict(
        backbone=dict(lr_mult=0.01, decay_mult=0.0)))))
    det_o = build_detector(cfg_o)
    det_o.to(DEV)
    tr_o = det_o.trainer(train_backbone=True)
    wds_o = tr_o.seg_wd.cpu()
    assert all(float(wds_o[i]) == 0.0 for i, n in enumerate(tr_o.layout) if n.startswith("backbone."))


def test_swin_full_drop_path_draws_all_blocks():
    keeps = []
    for _ in range(2):
        _, det = _tiny_detector(-1)
        tr = det.trainer(train_backbone=True, drop_path=True, seed=5)
        keeps.append([tr._drop_path_keep(BATCH).cpu() for _ in range(3)])
    rates = torch.linspace(0, DROP_PATH, NBLK, dtype=torch.float64)
    for a, b in zip(*keeps):
        assert tuple(a.shape) == (NBLK, 2, BATCH) and torch.equal(a, b)
        for j in range(NBLK):
            on = 1.0 / (1.0 - float(rates[j]))
            assert all(float(v) == 0.0 or abs(float(v) - on) < 1e-6 for v in a[j].flatten()), j
    assert bool((keeps[0][0][0] == 1.0).all())     # block 0: rate 0, never dropped
    assert any(bool((k == 0.0).any()) for k in keeps[0])
