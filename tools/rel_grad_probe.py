"""Times the relation branch's backward of the sibling head (labnotes R23) at B = 1 and the shapes of
an 800 x 1333 image:

  attention   pn_mha_bwd_keysplit_f32 beside pn_mha_bwd_f32 on the same unmasked inputs, ALTERNATING
              calls in one process, Nq = 100 against the three memory levels (1 050, 4 200, 16 700
              keys), with the largest difference between their outputs
  head        `BaselineHeadGrad` (forward_from_plan + backward, what `head_backward` runs) beside
              `SegmenterHeadGrad` (what `seg_backward` runs) on the same plan, for both
              `attn_bwd_algo` values
  full        the same two followed by `SegPixelDecoderGrad.forward` + `.backward` (what
              `full_backward` / `segmenter_backward` run)

HIP events around each call, 3 warm-up calls, median with min-max of `--iters` calls, `--repeats`
times (the R20.4 protocol); the spread of a comparison is the range of its per-repeat median ratios.

    python tools/rel_grad_probe.py [--iters 20] [--repeats 3] [--out profiles/rel_grad.json]
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
LEVELS = (1050, 4200, 16700)


def attention_case(hip, Nk, Nq=100, B=1, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + Nk)
    r = lambda n: torch.randn(B * n, 256, generator=g, device=DEV)
    q, k, v, do = r(Nq), r(Nk), r(Nk), r(Nq)
    outs = [[torch.empty_like(t) for t in (q, k, v)] for _ in range(2)]
    ks_scr = torch.empty(hip.mha_bwd_keysplit_scratch_floats(B, Nq, Nk), device=DEV)
    scr = torch.empty(hip.mha_bwd_scratch_floats(B, Nq, Nk), device=DEV)
    scale = 32 ** -0.5
    new = lambda: hip.mha_bwd_keysplit(q, k, v, do, *outs[0], ks_scr, B, Nq, Nk, scale)
    old = lambda: hip.mha_bwd(q, k, v, do, *outs[1], scr, B, Nq, Nk, scale)
    return new, old, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--attention-only", action="store_true")
    args = ap.parse_args()
    from pairnet_amd import hip
    res = dict(chunk=hip.MHA_KEYSPLIT_CHUNK, attention={}, runs=[])
    cases = {}
    with torch.no_grad():
        for Nk in LEVELS:
            new, old, outs = attention_case(hip, Nk)
            new(), old()
            torch.cuda.synchronize()
            diff = [float((a - b).abs().max()) for a, b in zip(*outs)]
            scale = [float(b.abs().max()) for b in outs[1]]
            res["attention"][str(Nk)] = dict(
                max_abs_difference=dict(zip(("dq", "dk", "dv"), diff)),
                max_abs=dict(zip(("dq", "dk", "dv"), scale)),
                scratch_floats=dict(keysplit=hip.mha_bwd_keysplit_scratch_floats(1, 100, Nk),
                                    mha_bwd=hip.mha_bwd_scratch_floats(1, 100, Nk)), runs=[])
            cases[Nk] = (new, old)
        for rep in range(args.repeats):
            for Nk in LEVELS:
                a, b = timed_alternating(*cases[Nk], args.iters)
                res["attention"][str(Nk)]["runs"].append(dict(keysplit=a, mha_bwd=b))
                print("repeat %d Nk %5d: keysplit %.3f ms (%.3f-%.3f), mha_bwd %.3f ms (%.3f-%.3f), "
                      "ratio %.2f" % (rep, Nk, a["median"], a["min"], a["max"], b["median"], b["min"],
                                      b["max"], b["median"] / a["median"]), flush=True)
    for Nk in LEVELS:
        e = res["attention"][str(Nk)]
        e["mha_bwd_over_keysplit"] = [r["mha_bwd"]["median"] / r["keysplit"]["median"]
                                      for r in e["runs"]]
    if not args.attention_only:
        tapes(args, res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def tapes(args, res):
    from helpers import baseline_cfg, oracle_baseline_head
    from oracle import seeded
    from pairnet_amd import (BaselineHeadGrad, CrossHeadBaseline, SegmenterHeadGrad,
                             SegPixelDecoderGrad)
    B, H, W, n_obj = 1, 800, 1333, 12
    _, sd, _ = oracle_baseline_head(1234)
    head = CrossHeadBaseline(**baseline_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    head.return_all_layers = True
    feats = [f.to(DEV) for f in seeded.seeded_feats(99, B, H, W)]
    head.forward(feats, [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4)])
    pl = head._last_plan
    g = torch.Generator().manual_seed(1)
    rows = torch.cat([torch.randperm(100, generator=g)[:n_obj].sort()[0] + l * 100 for l in range(9)])
    grads = dict(cls=torch.randn(9, B, 100, 134, generator=g).to(DEV),
                 mask=torch.randn(9 * n_obj, pl.hw2[0], pl.hw2[1], generator=g).to(DEV),
                 mask_rows=rows.long().to(DEV), rel=torch.randn(B, 100, 57, generator=g).to(DEV),
                 subject_scores=torch.randn(B, 100, 100, generator=g).to(DEV),
                 object_scores=torch.randn(B, 100, 100, generator=g).to(DEV))
    seg = {k: grads[k] for k in ("cls", "mask", "mask_rows")}
    full, parent, pdt = BaselineHeadGrad(head), SegmenterHeadGrad(head), SegPixelDecoderGrad(head)

    def head_backward():
        full.forward_from_plan(pl)
        return full.backward(grads, counts=[n_obj])

    def seg_backward():
        parent.forward_from_plan(pl)
        return parent.backward(seg, counts=[n_obj])

    def through(fn):
        def run():
            dmem, dMF, _ = fn()
            pdt.forward(feats)
            pdt.backward(dmem, dMF)
        return run

    res["shape"] = dict(B=B, N=list(pl.N), hw2=list(pl.hw2), objects=n_obj)
    iters = max(3, args.iters // 4)
    for rep in range(args.repeats):
        run = {}
        for algo in BaselineHeadGrad.ATTN_BWD_ALGOS:
            full.attn_bwd_algo = algo
            run["head_backward_" + algo], run["seg_backward_beside_" + algo] = timed_alternating(
                head_backward, seg_backward, iters, warmup=1)
            run["full_backward_" + algo], run["segmenter_backward_beside_" + algo] = \
                timed_alternating(through(head_backward), through(seg_backward), iters, warmup=1)
        res["runs"].append(run)
        print(rep, {k: "%.2f ms (%.2f-%.2f)" % (v["median"], v["min"], v["max"])
                    for k, v in run.items()}, flush=True)


if __name__ == "__main__":
    main()
