"""Times the segmentation-loss backward at the production shape (labnotes R18.4): L 9, B 2, Q 100,
200 x 334 mask logits, 20 objects per image (M = 360 compact rows).

  kernels           pn_mask_embed_grad_f32 and pn_mask_feature_grad_f32, each alone
  torch ops         the same two products the only way they could be had before: index_select of
                    the rows, transpose, matmul per image on the device (fp32)
  backward          the whole `SegmenterHeadGrad.backward` (heads + nine layers) at an 800 x 1333
                    pyramid, gradients of `seg_losses` on the head's own outputs

HIP events around each call, warm-up first, median with min-max of `--iters` calls, `--repeats` times.

    python tools/seg_grad_probe.py [--iters 30] [--repeats 3] [--out FILE.json] [--no-backward]
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


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--no-backward", action="store_true")
    args = ap.parse_args()
    from pairnet_amd import hip
    L, B, Q, h, w, n = 9, 2, 100, 200, 334, 20
    P, counts = h * w, [n] * B
    M = L * n * B
    g = torch.Generator().manual_seed(0)
    G = torch.randn(M, P, generator=g).to(DEV)
    MF = torch.randn(B, P, 256, generator=g).to(DEV)
    me = torch.randn(L * B * Q, 256, generator=g).to(DEV)
    rows = torch.cat([torch.randperm(Q, generator=g)[:n].sort()[0] + (l * B + b) * Q
                      for l in range(L) for b in range(B)]).to(DEV)
    table, T = hip.mask_grad_table(L, counts)
    table = table.to(DEV)
    dme, dMF = torch.empty(M, 256, device=DEV), torch.empty(B, P, 256, device=DEV)
    scratch = torch.empty(hip.mask_embed_grad_scratch_floats(T, P), device=DEV)
    img = torch.arange(M, device=DEV) % (n * B) // n
    sel = [torch.nonzero(img == b).view(-1) for b in range(B)]

    def k1():
        hip.mask_embed_grad(G, MF, rows, table, T, dme, scratch)

    def k2():
        hip.mask_feature_grad(G, me, rows, table, T, dMF)

    t_dme, t_dMF = torch.empty_like(dme), torch.empty_like(dMF)

    def torch_dme():
        for b in range(B):
            t_dme[sel[b]] = G.index_select(0, sel[b]) @ MF[b]

    def torch_dmf():
        for b in range(B):
            Gb = G.index_select(0, sel[b])
            torch.matmul(Gb.t(), me.index_select(0, rows.index_select(0, sel[b])), out=t_dMF[b])

    k1(), k2(), torch_dme(), torch_dmf()
    torch.cuda.synchronize()
    print("kernels against torch ops: dme %.2e, dMF %.2e (max abs difference; max |dme| %.1f)"
          % (float((dme - t_dme).abs().max()), float((dMF - t_dMF).abs().max()),
             float(t_dme.abs().max())))
    fns = dict(mask_embed_grad=k1, mask_feature_grad=k2, torch_mask_embed_grad=torch_dme,
               torch_mask_feature_grad=torch_dmf)
    if not args.no_backward:
        from helpers import baseline_cfg, oracle_baseline_head
        from oracle import seeded
        from pairnet_amd import CrossHeadBaseline, SegmenterHeadGrad
        _, sd, _ = oracle_baseline_head(1234)
        head = CrossHeadBaseline(**baseline_cfg())
        head.load_state_dict(sd)
        head.to(DEV)
        head.return_all_layers = True
        H, W = 800, 1333
        feats = [f.to(DEV) for f in seeded.seeded_feats(99, B, H, W)]
        cls, masks = head.forward(feats, [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4)] * B)
        hh, ww = masks["mask"].shape[-2:]
        gt_labels = [torch.randint(0, 133, (n,), generator=g) for _ in range(B)]
        gt_masks = [(torch.rand(n, hh * 2, ww * 2, generator=g) > 0.7).to(torch.uint8) for _ in range(B)]
        grads = {}
        head.seg_losses(cls, masks, gt_labels, gt_masks, [dict()] * B, grads=grads, seed=1)
        tape = SegmenterHeadGrad(head)
        tape.forward_from_plan(head._last_plan)
        fns["backward"] = lambda: tape.backward(grads, counts=counts)
        fns["forward_from_plan"] = lambda: tape.forward_from_plan(head._last_plan)
    res = dict(shape=dict(L=L, B=B, Q=Q, h=h, w=w, objects=n, M=M), runs=[])
    for rep in range(args.repeats):
        run = {k: timed(f, args.iters) for k, f in fns.items()}
        res["runs"].append(run)
        print(rep, {k: "%.3f ms (%.3f-%.3f)" % (v["median"], v["min"], v["max"]) for k, v in run.items()},
              flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
