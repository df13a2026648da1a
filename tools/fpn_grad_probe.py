"""Times the backward of the pixel decoder's FPN branch (labnotes R20) at B = 1 and the feature
shapes of an 800 x 1333 image (C2 200 x 334 over C3 100 x 167):

  kernels     every step of `SegPixelDecoderGrad.backward`'s branch, and their sum
  adjoint     pn_bilinear_nhwc_bwd_f32 beside torch's upsample_bilinear2d backward (NCHW, fp32)
  groupnorm   pn_groupnorm_act_nhwc_bwd_f32 beside the composition it replaces (relu_bwd,
              pn_groupnorm_nhwc_bwd_f32, two colsum), same inputs, ALTERNATING calls
  data grad   the 3x3's data gradient as the direct implicit GEMM and as Winograd F(4x4, 3x3), both
              on the reversed weight
  backward    the whole `SegPixelDecoderGrad.backward` beside `PixelDecoderGrad.backward` on the
              same dmem

HIP events around each call, warm-up first, median with min-max of `--iters` calls, `--repeats`
times; the spread of a comparison is the range of its per-repeat median ratios.

    python tools/fpn_grad_probe.py [--iters 20] [--repeats 3] [--out profiles/fpn_grad.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"


def _event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def _stat(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return _stat([_event_ms(fn) for _ in range(iters)])


def timed_alternating(fa, fb, iters, warmup=3):
    """a, b, a, b, ...: both see the same clocks and the same cache history."""
    for _ in range(warmup):
        fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(iters):
        ta.append(_event_ms(fa))
        tb.append(_event_ms(fb))
    return _stat(ta), _stat(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    from helpers import baseline_cfg, oracle_baseline_head
    from oracle import seeded
    from pairnet_amd import CrossHeadBaseline, PixelDecoderGrad, SegPixelDecoderGrad, hip
    B, H, W = 1, 800, 1333
    _, sd, _ = oracle_baseline_head(1234)
    head = CrossHeadBaseline(**baseline_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    feats = [f.to(DEV) for f in seeded.seeded_feats(99, B, H, W)]
    tape, parent = SegPixelDecoderGrad(head), PixelDecoderGrad(head)
    mem, MF = tape.forward(feats)
    parent.forward(feats)
    s, t, w, pd = tape.t["fpn"], tape.t, head.w, tape.PD
    (H2, W2), (h2, w2), SN, G = s["hw2"], t["shapes"][2], t["SN"], head.gn_groups
    HW2 = H2 * W2
    g = torch.Generator().manual_seed(0)
    dmem = torch.randn(tuple(mem.shape), generator=g).to(DEV)
    dMF = torch.randn(tuple(MF.shape), generator=g).to(DEV)
    E = tape._E
    grads = tape.grads
    scratch, stats = hip.groupnorm_act_bwd_scratch(B, HW2, G, DEV), E(B * G * 4)
    dY = torch.randn(B * HW2, 256, generator=g).to(DEV)
    dc3 = torch.randn(B, H2, W2, 256, generator=g).to(DEV)
    dT = torch.randn(B, H2, W2, 256, generator=g).to(DEV)
    wb = E(256 * 9 * 256)
    hip.conv_weight_bwd_layout(w[pd + "output_convs.0.conv.weight"], wb, 256, 9, 256)
    rows_per = min(H2, 8)
    part = E(B * ((H2 + rows_per - 1) // rows_per), 256 * 9 * 256)
    dwp, out_d, out_w = E(256 * 9 * 256), E(B, H2, W2, 256), E(B, H2, W2, 256)
    U = hip.winograd43_weights(wb.view(256, 3, 3, 256).permute(0, 3, 1, 2).contiguous())
    Tn = B * ((H2 + 3) // 4) * ((W2 + 3) // 4)
    wV, wM = E(36 * Tn * 256), E(36 * Tn * 256)
    dsum = dmem.clone()
    # the composition pn_groupnorm_act_nhwc_bwd_f32 replaces, on the kernels the parent has
    c_dy, c_dx, c_gx, c_st = E(B * HW2, 256), E(B * HW2, 256), E(B * HW2, 256), E(B * G * 4)
    c_dg, c_db = E(256), E(256)

    def gn_composition():
        hip.relu_bwd(dY, s["Y"].view(-1, 256), c_dy)
        hip.groupnorm_nhwc_bwd(s["c3"], c_dy, w[pd + "output_convs.0.gn.weight"], c_dx, c_gx, c_st, B,
                               HW2, G, HW2 * 256, HW2 * 256)
        hip.colsum(c_gx, c_dg)
        hip.colsum(c_dy, c_db)

    n_dx, n_dg, n_db = E(B * HW2, 256), E(256), E(256)

    def gn_entry():
        hip.groupnorm_act_nhwc_bwd(s["c3"], dY, s["Y"], w[pd + "output_convs.0.gn.weight"], n_dx, n_dg,
                                   n_db, stats, scratch, B, HW2, G, True, False, HW2 * 256, HW2 * 256)

    def wgrad():
        hip.conv_wgrad(dc3, s["T"], part, B, H2, W2, H2, W2, 256, 256, 3, 1, 1, rows_per)
        hip.colsum(part, dwp)
        grads[pd + "output_convs.0.conv.weight"].copy_(dwp.view(256, 3, 3, 256).permute(0, 3, 1, 2))

    def dgrad_direct():
        hip.conv2d_ex(dc3, wb.view(256, 9 * 256), None, None, out_d, B, H2, W2, 256, 256, 3, 3, 1, 1)

    def dgrad_winograd():
        hip.conv3x3_winograd43(dc3, U, None, out_w, wV, wM, B, H2, W2, 256, 256, False)

    def adjoint():
        hip.bilinear_nhwc_bwd(dT, dsum[:, t["start"][2]:], B, h2, w2, H2, W2, 256, True, HW2 * 256,
                              SN * 256)

    x_t = torch.zeros(B, 256, h2, w2, device=DEV, requires_grad=True)
    g_t = dT.permute(0, 3, 1, 2).contiguous()

    def adjoint_torch():
        y = torch.nn.functional.interpolate(x_t, size=(H2, W2), mode="bilinear", align_corners=False)
        torch.autograd.grad(y, x_t, g_t)

    with torch.no_grad():
        gn_composition(), gn_entry(), dgrad_direct(), dgrad_winograd()
        torch.cuda.synchronize()
        check = dict(gn_dx=float((n_dx - c_dx).abs().max()), gn_dgamma=float((n_dg - c_dg).abs().max()),
                     gn_dbeta=float((n_db - c_db).abs().max()), gn_dx_scale=float(c_dx.abs().max()),
                     dgrad_winograd_vs_direct=float((out_w - out_d).abs().max()),
                     dgrad_scale=float(out_d.abs().max()))
    print("agreement (max abs difference):", check, flush=True)
    nd = torch.no_grad()
    steps = dict(
        lin_bwd_mask_feature=lambda: tape._lin_bwd(dMF.view(-1, 256), s["Y"].view(-1, 256),
                                                   w[pd + "mask_feature.weight"], grads,
                                                   pd + "mask_feature.weight", pd + "mask_feature.bias"),
        gn_relu_bwd_output_conv=gn_entry, conv_wgrad_colsum_permute=wgrad,
        weight_bwd_layout=lambda: hip.conv_weight_bwd_layout(w[pd + "output_convs.0.conv.weight"],
                                                             wb, 256, 9, 256),
        dgrad_winograd43_with_weight_transform=lambda: (
            hip.winograd43_weights(wb.view(256, 3, 3, 256).permute(0, 3, 1, 2).contiguous()),
            dgrad_winograd()),
        gn_bwd_lateral=lambda: tape._gn_bwd(s["lat"], dT, None, pd + "lateral_convs.0.gn.", grads, B,
                                            HW2, scratch, stats),
        lin_bwd_lateral_no_dx=lambda: tape._lin_bwd(dY, s["rows"][0], w[pd + "lateral_convs.0.conv.weight"],
                                                    grads, pd + "lateral_convs.0.conv.weight", None,
                                                    need_dx=False),
        bilinear_nhwc_bwd=adjoint)
    res = dict(shape=dict(B=B, H2=H2, W2=W2, h2=h2, w2=w2, SN=SN, G=G), agreement=check, runs=[])
    for rep in range(args.repeats):
        with nd:
            run = {k: timed(f, args.iters) for k, f in steps.items()}
            run["branch_sum_of_medians"] = sum(v["median"] for v in run.values())
            run["gn_entry"], run["gn_composition"] = timed_alternating(gn_entry, gn_composition,
                                                                       args.iters)
            run["dgrad_direct_alt"], run["dgrad_winograd43"] = timed_alternating(
                dgrad_direct, dgrad_winograd, args.iters)
            run["seg_backward"], run["parent_backward"] = timed_alternating(
                lambda: tape.backward(dmem, dMF), lambda: parent.backward(dmem), max(3, args.iters // 4),
                warmup=1)
        run["adjoint_torch"] = timed(adjoint_torch, args.iters)
        res["runs"].append(run)
        print(rep, {k: ("%.3f ms (%.3f-%.3f)" % (v["median"], v["min"], v["max"])
                        if isinstance(v, dict) else "%.3f ms" % v) for k, v in run.items()}, flush=True)
    ratios = lambda a, b: [r[a]["median"] / r[b]["median"] for r in res["runs"]]
    res["ratios"] = dict(gn_composition_over_entry=ratios("gn_composition", "gn_entry"),
                         dgrad_direct_over_winograd43=ratios("dgrad_direct_alt", "dgrad_winograd43"),
                         adjoint_torch_over_kernel=ratios("adjoint_torch", "bilinear_nhwc_bwd"),
                         seg_backward_over_parent=ratios("seg_backward", "parent_backward"))
    print("ratios per repeat:", res["ratios"], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
