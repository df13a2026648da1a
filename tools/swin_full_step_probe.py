"""Times the all-stage Swin training step and the patch-merging backward kernel (labnotes R25) at
B = 1 and the shapes of an 800 x 1333 image, Swin-B with window 12:

  merge   pn_patch_merge_ln_bwd_f32 (+ the pn_colsum_f32 of its partials) beside the same operator
          composed from torch ops -- index_select (the 2x2 gather, a zero row for the padding),
          native_layer_norm (the moments), native_layer_norm_backward, index_copy_ (the scatter) --
          ALTERNATING calls in one process, at the three merge shapes 200x334x128, 100x167x256,
          50x84x512; each case records the largest difference between the two results and the
          bytes the kernel has to move (dy, x, dx, gamma once).
  step    one `TailTrainer.step` from the image with `frozen_stages=3` (SwinBackboneGrad: the last
          stage) and with `frozen_stages=-1` (SwinStagesGrad: every stage, the patch mergings, the
          patch embedding), each on its own detector with the same seeded weights, alternating;
          the peak device memory of one step of each (torch's allocator, after the trainer is built).

HIP events around each call, 3 warm-up calls, median with min-max of `--iters` calls, `--repeats`
times.  There is no parent figure for the `-1` step: the figures are recorded, not gated.

    python tools/swin_full_step_probe.py [--iters 10] [--repeats 3] [--out profiles/swin_full_step.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from fpn_grad_probe import timed_alternating  # noqa: E402

DEV = "cuda:0"
MERGES = ((200, 334, 128), (100, 167, 256), (50, 84, 512))
EPS = 1e-5


def merge_case(hip, H, W, C, seed=0):
    """(new, old, results): the HIP kernel and the torch composition on the same operands."""
    B, H2, W2 = 1, (H + 1) // 2, (W + 1) // 2
    rows, n = B * H2 * W2, B * H * W
    g = torch.Generator(device=DEV).manual_seed(seed + C)
    x = torch.randn(n, C, generator=g, device=DEV) * 2.0 + 0.3
    dy = torch.randn(rows, 4 * C, generator=g, device=DEV)
    gamma = torch.rand(4 * C, generator=g, device=DEV) + 0.5
    beta = torch.zeros(4 * C, device=DEV)
    nblk = hip.patch_merge_ln_bwd_nblocks(B, H, W)
    dx, part, gb = (torch.empty(n, C, device=DEV), torch.empty(nblk, 8 * C, device=DEV),
                    torch.empty(8 * C, device=DEV))

    def new():
        hip.patch_merge_ln_bwd(dy, x, gamma, dx, part, B, H, W, C, EPS)
        hip.colsum(part, gb)

    # the gather as an index list over the rows of x, row n = the zero padding
    y2, x2, q = torch.meshgrid(torch.arange(H2), torch.arange(W2), torch.arange(4), indexing="ij")
    yy, xx = 2 * y2 + q // 2, 2 * x2 + q % 2
    idx = torch.where((yy < H) & (xx < W), yy * W + xx, torch.full_like(yy, n)).reshape(-1).to(DEV)
    xpad = torch.cat([x, torch.zeros(1, C, device=DEV)])
    out = {}

    def old():
        gath = xpad.index_select(0, idx).view(rows, 4 * C)
        _, mean, rstd = torch.ops.aten.native_layer_norm(gath, [4 * C], gamma, beta, EPS)
        dg, dgam, dbet = torch.ops.aten.native_layer_norm_backward(
            dy, gath, [4 * C], mean, rstd, gamma, beta, [True, True, True])
        out["dx"] = torch.zeros(n + 1, C, device=DEV).index_copy_(0, idx, dg.view(-1, C))[:n]
        out["dgamma"], out["dbeta"] = dgam, dbet

    new(), old()
    torch.cuda.synchronize()
    diff = dict(dx=float((dx - out["dx"]).abs().max()), dx_max=float(out["dx"].abs().max()),
                dgamma=float((gb[:4 * C] - out["dgamma"]).abs().max()),
                dgamma_max=float(out["dgamma"].abs().max()),
                dbeta=float((gb[4 * C:] - out["dbeta"]).abs().max()),
                dbeta_max=float(out["dbeta"].abs().max()))
    nbytes = 4 * (rows * 4 * C + 2 * n * C + 4 * C + nblk * 8 * C)
    return new, old, diff, nbytes, nblk


def merges(args, res, hip):
    table = {}
    for H, W, C in MERGES:
        new, old, diff, nbytes, nblk = merge_case(hip, H, W, C)
        name = "%dx%dx%d" % (H, W, C)
        table[name] = dict(H=H, W=W, C=C, workgroups=nblk, kernel_bytes=nbytes,
                           max_abs_difference=diff, runs=[], fns=(new, old))
        print("%-14s %d workgroups, %.1f MB; difference from the torch composition %s"
              % (name, nblk, nbytes / 1e6, {k: "%.2e" % v for k, v in diff.items()}), flush=True)
    for rep in range(args.repeats):
        for name, e in table.items():
            a, b = timed_alternating(*e["fns"], args.iters)
            e["runs"].append(dict(hip=a, torch_ops=b))
            print("repeat %d %-14s hip %.3f ms (%.3f-%.3f) = %.0f GB/s, torch ops %.3f ms (%.3f-%.3f), "
                  "ratio %.2f" % (rep, name, a["median"], a["min"], a["max"],
                                  e["kernel_bytes"] / a["median"] / 1e6, b["median"], b["min"],
                                  b["max"], b["median"] / a["median"]), flush=True)
    for e in table.values():
        del e["fns"]
        e["torch_ops_over_hip"] = [r["torch_ops"]["median"] / r["hip"]["median"] for r in e["runs"]]
    res["merge"] = table


def step(args, res):
    from pairnet_amd import build_detector, pairnet_swin
    H, W, n_obj = 800, 1333, 12
    g = torch.Generator().manual_seed(11)
    img = torch.randn(1, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4, batch_input_shape=(H, W))]
    gt_labels = [torch.randint(0, 133, (n_obj,), generator=g)]
    gt_masks = [(torch.rand(n_obj, H // 2, W // 2, generator=g) > 0.6).to(torch.uint8).to(DEV)]
    pairs = torch.randperm(n_obj * n_obj, generator=g)[:8]
    gt_rels = [torch.stack([pairs // n_obj, pairs % n_obj,
                            torch.randint(1, 57, (8,), generator=g)], 1)]
    gt_rels = [r[r[:, 0] != r[:, 1]] for r in gt_rels]
    runs, info = {}, {}
    for f in (3, -1):
        cfg = pairnet_swin("B")
        cfg["backbone"]["frozen_stages"] = f
        det = build_detector(cfg)
        det.bbox_head.init_weights(seed=4)
        det.to(DEV)
        tr = det.trainer(train_backbone=True, decay_mult={"backbone.": 0.0})
        tr.step(img, metas, gt_rels, gt_labels, gt_masks)               # (plans, first launches)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = tr.step(img, metas, gt_rels, gt_labels, gt_masks)
        torch.cuda.synchronize()
        info[f] = dict(tape=type(tr.bb_tape).__name__, parameters=int(tr.n),
                       backbone_parameters=int(tr.bb_tape.flat_numel),
                       allocated_before_step_bytes=int(base),
                       peak_allocated_in_step_bytes=int(torch.cuda.max_memory_allocated()),
                       grad_norm=float(out["grad_norm"]))
        runs[f] = (lambda t=tr: t.step(img, metas, gt_rels, gt_labels, gt_masks))
        print("frozen_stages=%d: %s, %.1f M parameters (%.1f M backbone), peak %.2f GB in a step "
              "(%.2f GB before it), grad_norm %.4g"
              % (f, info[f]["tape"], tr.n / 1e6, tr.bb_tape.flat_numel / 1e6,
                 info[f]["peak_allocated_in_step_bytes"] / 2 ** 30, base / 2 ** 30,
                 info[f]["grad_norm"]), flush=True)
    res["step"] = dict(shape=dict(B=1, H=H, W=W, objects=n_obj, relations=int(gt_rels[0].shape[0])),
                       variants={str(f): v for f, v in info.items()}, runs=[])
    for rep in range(args.repeats):
        a, b = timed_alternating(runs[3], runs[-1], args.iters)
        res["step"]["runs"].append({"3": a, "-1": b})
        print("repeat %d step: frozen_stages=3 %.2f ms (%.2f-%.2f), frozen_stages=-1 %.2f ms "
              "(%.2f-%.2f), ratio %.2f" % (rep, a["median"], a["min"], a["max"], b["median"],
                                           b["min"], b["max"], b["median"] / a["median"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--merge-only", action="store_true")
    args = ap.parse_args()
    from pairnet_amd import hip
    res = dict(image=[800, 1333], backbone="Swin-B, window 12")
    with torch.no_grad():
        merges(args, res, hip)
        if not args.merge_only:
            step(args, res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
