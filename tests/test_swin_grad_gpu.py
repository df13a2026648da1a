"""GPU: the Swin backbone's last-stage backward (csrc/swin_grad.hip, grad.py SwinBackboneGrad) and its
training step (TailTrainer with a SwinTransformerHip backbone) against autograd through oracle/swin.py
in float64.  Tolerance as tests/test_grad_gpu.py: 1e-4 of each tensor's largest entry."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.swin import (OracleSwin, relative_position_index, seeded_swin_state, shift_mask,
                         windows_of)
from test_grad_gpu import _compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def R(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---------------------------------------------------------------- kernel level
def _window_core(grid, table, B, hp, wp, C, heads, ws, shift):
    """(Shifted-)window attention of ShiftWindowMSA after its qkv Linear, on the padded qkv grid
    [B, hp, wp, 3C] -> the attention output on the padded grid [B, hp, wp, C]."""
    N = ws * ws
    g = torch.roll(grid, (-shift, -shift), (1, 2)) if shift else grid
    win = windows_of(g.contiguous(), ws)
    nb = win.shape[0]
    q, k, v = win.reshape(nb, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    attn = (q * 32 ** -0.5) @ k.transpose(-2, -1)
    attn = attn + table[relative_position_index(ws).view(-1)].view(N, N, heads).permute(2, 0, 1)
    if shift:
        mask = shift_mask(hp, wp, ws, shift).to(attn.dtype)
        nw = mask.shape[0]
        attn = (attn.view(nb // nw, nw, heads, N, N) + mask[None, :, None]).view(nb, heads, N, N)
    o = (attn.softmax(-1) @ v).transpose(1, 2).reshape(nb, N, C)
    y = o.view(B, hp // ws, wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, hp, wp, C)
    return torch.roll(y, (shift, shift), (1, 2)) if shift else y


@pytest.mark.parametrize("B,H,W,heads,ws,shift,saved", [
    (2, 9, 10, 2, 7, 0, True), (2, 9, 10, 2, 7, 3, True), (2, 14, 25, 2, 12, 0, True),
    (2, 14, 25, 2, 12, 6, True), (2, 6, 8, 2, 12, 6, True), (2, 6, 8, 2, 12, 0, False),
    (2, 14, 25, 2, 12, 6, False)])
def test_window_attention_bwd_matches_autograd(B, H, W, heads, ws, shift, saved):
    from pairnet_amd import hip
    C = heads * 32
    hp, wp = -(-H // ws) * ws, -(-W // ws) * ws
    nrel = (2 * ws - 1) ** 2
    qkv, bias = R(B * H * W, 3 * C, seed=1), R(3 * C, seed=2, scale=0.5)
    table, G = R(nrel, heads, seed=3, scale=0.5), R(B * H * W, C, seed=4)
    # oracle: the padded grid (real rows = qkv, padding rows = the qkv bias) as the leaf
    grid = bias.double().expand(B, hp, wp, 3 * C).clone()
    grid[:, :H, :W] = qkv.double().view(B, H, W, 3 * C)
    grid.requires_grad_(True)
    tab = table.double().requires_grad_(True)
    y = _window_core(grid, tab, B, hp, wp, C, heads, ws, shift)[:, :H, :W].reshape(B * H * W, C)
    (y * G.double()).sum().backward()

    qkv_d, bias_d, tab_d = qkv.to(DEV), bias.to(DEV), table.t().contiguous().to(DEV)
    out = torch.empty(B * H * W, C, device=DEV)
    hip.window_attention(qkv_d, bias_d, tab_d, out, B, H, W, C, heads, ws, shift)
    report = []
    _compare("out", out, y, report)
    dqkv = torch.full((B * hp * wp, 3 * C), float("nan"), device=DEV)
    part = torch.empty(hip.window_partials_rows(B, H, W, ws), heads * nrel, device=DEV)
    hip.window_attention_bwd(qkv_d, bias_d, tab_d, G.to(DEV), dqkv, part, B, H, W, C, heads, ws,
                             shift, out=out if saved else None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dqkv).all())           # every padded-grid row is written
    ref = grid.grad.view(B, hp, wp, 3 * C)
    got = dqkv.view(B, hp, wp, 3 * C).cpu()
    for i, nm in enumerate("qkv"):
        sl = slice(i * C, (i + 1) * C)
        _compare("d" + nm, got[:, :H, :W, sl], ref[:, :H, :W, sl], report)
    pad = torch.ones(B, hp, wp, dtype=torch.bool)
    pad[:, :H, :W] = False
    if bool(pad.any()):
        _compare("d bias (padding rows)", got[pad].sum(0), ref[pad].sum(0), report)
    dtab = torch.empty(heads * nrel, device=DEV)
    hip.colsum(part, dtab)
    _compare("d table", dtab.view(heads, nrel).t(), tab.grad, report)


@pytest.mark.parametrize("C", [96, 768, 1024, 1536])
def test_layernorm_rows_bwd_and_gelu_match_autograd(C):
    from pairnet_amd import hip
    rows = 37
    x = (R(rows, C, seed=1, scale=2.0) + 0.3).double().requires_grad_(True)
    gm, bt, dy = R(C, seed=2).double() + 1.0, R(C, seed=3).double(), R(rows, C, seed=4).double()
    gm.requires_grad_(True)
    y = F.layer_norm(x, (C,), gm, bt, 1e-5)
    (y * dy).sum().backward()
    dx, gx = torch.empty(rows, C, device=DEV), torch.empty(rows, C, device=DEV)
    hip.layernorm_rows_bwd(dy.float().to(DEV), x.detach().float().to(DEV), gm.detach().float().to(DEV),
                           dx, gx)
    report = []
    _compare("dx", dx, x.grad, report)
    _compare("d weight", gx.sum(0), gm.grad, report)
    # exact GELU and its derivative
    pre = R(rows, C, seed=5, scale=3.0).double().requires_grad_(True)
    h = F.gelu(pre)
    (h * dy).sum().backward()
    hd = torch.empty(rows, C, device=DEV)
    hip.gelu(pre.detach().float().to(DEV), hd)
    _compare("gelu", hd, h, report)
    dpre = dy.float().to(DEV)
    hip.gelu_bwd(dpre, pre.detach().float().to(DEV), dpre)     # (in place)
    _compare("gelu'", dpre, pre.grad, report)


# ---------------------------------------------------------------- stage tape
VARIANTS = {"B": dict(embed_dims=128, num_heads=(4, 8, 16, 32)),
            "L": dict(embed_dims=192, num_heads=(6, 12, 24, 48))}


@pytest.fixture(scope="module", params=["B", "L"])
def stage(request):
    from pairnet_amd import SwinBackboneGrad, SwinTransformerHip
    dims = dict(depths=(2, 2, 2, 2), window_size=12, **VARIANTS[request.param])
    oracle = OracleSwin(**dims)
    oracle.load_state_dict(seeded_swin_state(oracle, 7))
    swin = SwinTransformerHip(frozen_stages=3, **dims)
    swin.load_state_dict(oracle.state_dict())
    swin.to(DEV)
    return request.param, oracle, swin, SwinBackboneGrad(swin)


def _oracle_stage(oracle, x4, G, keep=None):
    """float64 copy of stages[3] + norm3 on x4 [B, h, w, C]; returns (c5 rows, grads, d x4)."""
    st, nm = copy.deepcopy(oracle.stages[3]).double(), copy.deepcopy(oracle.norm3).double()
    B, h, w, C = x4.shape
    x0 = x4.double().view(B, h * w, C).requires_grad_(True)
    x = x0
    for j, blk in enumerate(st.blocks):
        sa = 1.0 if keep is None else keep[j, 0].double().view(B, 1, 1)
        sf = 1.0 if keep is None else keep[j, 1].double().view(B, 1, 1)
        x = x + sa * blk.attn(blk.norm1(x), (h, w))
        x = x + sf * blk.ffn(blk.norm2(x))
    y = nm(x)
    (y * G.double().view(B, h * w, C)).sum().backward()
    grads = {"stages.3." + k: p.grad for k, p in st.named_parameters()}
    grads.update({"norm3." + k: p.grad for k, p in nm.named_parameters()})
    return y.detach(), grads, x0.grad


def _check_stage(tape, oracle, x4, keep, report):
    B, h, w, C = x4.shape
    G = R(B, h, w, C, seed=11)
    y, ref, dx_ref = _oracle_stage(oracle, x4, G, keep)
    c5 = tape.forward(x4.to(DEV), keep=keep)
    _compare("c5", c5.view(B, h * w, C), y, report)
    grads, dx = tape.backward(G.to(DEV).permute(0, 3, 1, 2), need_dx=True)
    names = [n for _, ns in tape.param_groups(tape.backbone) for n in ns]
    assert set(names) == set(ref) and len(names) == 28
    for n in names:
        _compare(n, grads[n], ref[n], report)
    _compare("d x4", dx, dx_ref.view(B, h, w, C), report)


def test_swin_stage_tape_matches_autograd(stage):
    name, oracle, swin, tape = stage
    C = swin.num_features[3]
    x4 = R(2, 14, 25, C, seed=9)
    report = []
    _check_stage(tape, oracle, x4, None, report)
    # bitwise reproducible: a second backward of the same tape
    first = tape.flat_grad.clone()
    tape.backward(R(2, 14, 25, C, seed=11).to(DEV).permute(0, 3, 1, 2))
    assert torch.equal(tape.flat_grad, first)


def test_swin_stage_tape_drop_path(stage):
    name, oracle, swin, tape = stage
    C = swin.num_features[3]
    x4 = R(2, 14, 25, C, seed=10)
    keep = torch.full((2, 2, 2), 1.0 / (1.0 - 0.3))
    keep[0, 0, 1] = 0.0          # image 1: block 0's attention branch dropped
    keep[1, 1, 0] = 0.0          # image 0: block 1's FFN branch dropped
    report = []
    _check_stage(tape, oracle, x4, keep, report)


def test_swin_stage_input_and_c5_match_inference(stage):
    name, oracle, swin, tape = stage
    img = R(2, 3, 128, 192, seed=12)
    feats = [f.clone() for f in swin(img.to(DEV))]
    x4 = tape.stage_input()
    with torch.no_grad():
        x, hw = oracle.patch_embed(img)
        for st in oracle.stages[:3]:
            for blk in st.blocks:
                x = blk(x, hw)
            x, hw = st.downsample(x, hw)
    want = x.view(2, hw[0], hw[1], -1)
    scale = float(want.abs().max())
    assert float((x4.cpu() - want).abs().max()) <= 2e-4 * scale
    c5 = tape.forward(x4)
    ref = feats[3].permute(0, 2, 3, 1)
    assert float((c5 - ref).abs().max()) <= 2e-4 * float(ref.abs().max())


# ---------------------------------------------------------------- the detector's training step
def test_swin_detector_train_step_from_the_image():
    from pairnet_amd import SwinTransformerHip, build_detector, pairnet_swin
    cfg = pairnet_swin("B")
    det = build_detector(cfg)
    det.bbox_head.init_weights(seed=4)
    det.to(DEV)
    g = torch.Generator().manual_seed(9)
    H, W = 128, 192
    img = torch.randn(1, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4, batch_input_shape=(H, W))]
    gt_labels = [torch.tensor([3, 17, 90, 120])]
    gt_masks = [(torch.rand(4, H, W, generator=g) > 0.6).numpy()]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 3, 17], [1, 0, 56]])]
    bb0 = {k: v.clone() for k, v in det.backbone.state_dict().items()}
    tr = det.trainer(train_backbone=True)
    assert tr.swin and tr.bb_tape is not None
    for _ in range(2):
        out = det.train_step(img, metas, gt_rels, None, gt_labels, gt_masks)
    assert all(np.isfinite(float(v)) for v in out.values()) and float(out["grad_norm"]) > 0
    tr.write_back()
    bb1 = det.backbone.state_dict()
    moved = {k for k in bb1 if not torch.equal(bb1[k].cpu(), bb0[k].cpu())}
    names = [n for _, ns in tr.bb_tape.param_groups(det.backbone) for n in ns]
    assert moved == set(names) and len(moved) == 28
    assert not any(k.startswith(("patch_embed", "stages.0", "stages.1", "stages.2", "norm0",
                                 "norm1", "norm2")) for k in moved)
    # optimizer groups: lr_mult 0.01, decay multiplier 1 for every backbone tensor
    lrs, wds = tr.seg_lr.cpu(), tr.seg_wd.cpu()
    for i, n in enumerate(tr.layout):
        if n.startswith("backbone."):
            assert abs(float(lrs[i]) - 0.01) < 1e-9 and float(wds[i]) == 1.0, n
    keep = tr._drop_path_keep(2).cpu()
    assert keep.shape == (2, 2, 2)
    for j, p in enumerate((0.3 * 22 / 23, 0.3)):
        assert all(float(v) in (0.0, pytest.approx(1 / (1 - p))) for v in keep[j].flatten())
    # a fresh backbone from the written-back state dict computes bit for bit what the trained one
    # computes: the packed copies (.s3 splits, transposed bias tables) were refreshed in place
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
    res = det.simple_test(img, metas)
    assert len(res) == 1
    # a state dict loaded behind the trainer's back: the trainer refuses to step
    det.backbone.load_state_dict(det.backbone.state_dict())
    with pytest.raises(RuntimeError, match="re-packed"):
        tr.step(img, metas, gt_rels, gt_labels, det._prepare_gt_masks(img, gt_masks))
    # the default keeps a Swin backbone frozen
    assert det.trainer().backbone is None
