"""Times what labnotes R30 reports for `PSGTrHead2`'s training step, at the production case of R29
(B 2, 800 x 1333, Q 100, C 133, Cr 56, 200 x 334 logits, (15, 14) objects, (30, 29) relations):

  heads     `pn_triplet_heads_bwd_f32` (csrc/tri_grad.hip: the three ragged class heads' backward in
            two launches, N = 200, widths 134 / 134 / 57) beside the COMPOSITION from the entries
            that were there before -- per head a zero-padded copy of the gradient and of the weight,
            two zero-filled padded gradient buffers, a row pad, a transpose, two GEMMs, a column sum
            and three adds (`Tape._lin_bwd` at a ragged output width) --
            both forms in the same run, alternating; and their largest difference;
  step      one `PSGTr2Trainer.step` from resident features and from the image (ResNet-50 stages 2-4
            trained), `masked_keysplit_min_keys` at its default, `deterministic` off and on
            alternating on one trainer;
  baseline  one `BaselineTrainer.step` from the same images in the same run, for orientation.

HIP events, 3 warm-up calls, 20 rounds, median with min-max (the R29.4 protocol).  Nothing here has a
pass / fail time.

    python tools/tri_step_probe.py [--iters 20] [--out profiles/tri_step.json]
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

from fpn_grad_probe import timed, timed_alternating  # noqa: E402

DEV = "cuda:0"
H, W = 800, 1333


def psgtr2_head():
    from helpers import oracle_psgtr2_head, psgtr2_cfg
    from pairnet_amd import PSGTrHead2
    _, sd, _ = oracle_psgtr2_head(1234)
    head = PSGTrHead2(**psgtr2_cfg())
    head.load_state_dict(sd)
    return head.to(DEV)


def heads(args, res):
    from pairnet_amd import PSGTr2HeadGrad, hip
    head = psgtr2_head()
    tape = PSGTr2HeadGrad(head)
    w = head.w
    N = 200
    g = torch.Generator(device=DEV).manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    names = ("sub_cls_embed", "obj_cls_embed", "rel_cls_embed")
    d = [r(N, w[n + ".weight"].shape[0]) for n in names]
    qn, pre = r(N, 256), r(N, 256)
    new_out = dict(dqn=pre.clone())
    for n in names:
        new_out[n + ".weight"] = torch.empty_like(w[n + ".weight"])
        new_out[n + ".bias"] = torch.empty_like(w[n + ".bias"])
    old_out = {k: torch.zeros_like(v) for k, v in new_out.items()}

    def new():
        hip.tri_heads_bwd(d[0], d[1], d[2], qn, *[w[n + ".weight"] for n in names], new_out["dqn"],
                          *[new_out[n + s] for n in names for s in (".weight", ".bias")], add=True)

    def composed():
        for dy, n in zip(d, names):
            tape._acc(old_out["dqn"], tape._lin_bwd(dy, qn, w[n + ".weight"], old_out, n + ".weight",
                                                    n + ".bias"))

    old_out["dqn"].copy_(pre)
    new(), composed()
    torch.cuda.synchronize()
    diff = {k: float((new_out[k] - old_out[k]).abs().max()) for k in new_out}
    a, b = timed_alternating(new, composed, args.iters)
    res["heads"] = dict(shape=dict(N=N, widths=[int(t.shape[1]) for t in d]), kernel=a, composed=b,
                        composed_over_kernel=b["median"] / a["median"], max_abs_difference=diff,
                        kernel_not_slower=a["median"] <= b["median"])
    print("heads: kernel %.4f ms (%.4f-%.4f), composed %.4f ms (%.4f-%.4f), ratio %.1f; max |diff| %.2e"
          % (a["median"], a["min"], a["max"], b["median"], b["min"], b["max"],
             b["median"] / a["median"], max(diff.values())), flush=True)
    del tape, head
    torch.cuda.empty_cache()


def batch():
    import tri_loss_ref as T
    case = T.tri_case(**T.PRODUCTION)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4, batch_input_shape=(H, W))] * 2
    gt_masks = [m.to(DEV).contiguous() for m in case["gt_masks"]]
    gt_labels = [t.long() for t in case["gt_labels"]]
    gt_rels = [t.long() for t in case["gt_rels"]]
    img = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(11)).to(DEV)
    return img, metas, gt_rels, gt_labels, gt_masks


def steps(args, res):
    from pairnet_amd import BaselineTrainer, CrossHeadBaseline, PSGTr2Trainer, ResNet50Hip
    from helpers import baseline_cfg, oracle_baseline_head
    img, metas, gt_rels, gt_labels, gt_masks = batch()
    res["step"] = dict(shape=dict(B=2, H=H, W=W, objects=[int(t.numel()) for t in gt_labels],
                                  relations=[int(t.shape[0]) for t in gt_rels]))
    bb = ResNet50Hip().to(DEV)
    feats = [f.clone(memory_format=torch.preserve_format) for f in bb(img)]
    for scope, x, backbone in (("feats", feats, None), ("image", img, bb)):
        tr = PSGTr2Trainer(psgtr2_head(), backbone=backbone)

        def variant(det, tr=tr, x=x):
            def run():
                tr.deterministic = tr.pd_tape.deterministic = det
                tr.step(x, metas, gt_rels, gt_labels, gt_masks)
            return run

        a, b = timed_alternating(variant(False), variant(True), args.iters)
        res["step"][scope] = dict(atomics=a, deterministic=b, parameters=int(tr.n),
                                  min_keys=tr.tape.masked_keysplit_min_keys,
                                  assign_status_last=int(tr._guard[0]))
        print("step from %s: %.2f ms (%.2f-%.2f), deterministic %.2f ms (%.2f-%.2f); status %d"
              % (scope, a["median"], a["min"], a["max"], b["median"], b["min"], b["max"],
                 res["step"][scope]["assign_status_last"]), flush=True)
        del tr
        torch.cuda.empty_cache()
    # ---- the sibling head's step on the same images, for orientation ----
    _, sd, _ = oracle_baseline_head(1234)
    head = CrossHeadBaseline(**baseline_cfg())
    head.load_state_dict(sd)
    tr = BaselineTrainer(head.to(DEV), backbone=ResNet50Hip().to(DEV))
    run = lambda: tr.step(img, metas, gt_rels, gt_labels, gt_masks)
    a = timed(run, args.iters)
    res["baseline_step_image"] = dict(a, assign_status_last=int(tr._guard[0]), parameters=int(tr.n))
    print("BaselineTrainer step from the image: %.2f ms (%.2f-%.2f)" % (a["median"], a["min"], a["max"]),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--heads-only", action="store_true")
    args = ap.parse_args()
    res = {}
    with torch.no_grad():
        heads(args, res)
        if not args.heads_only:
            steps(args, res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
