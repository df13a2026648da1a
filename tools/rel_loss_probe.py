"""Times the sibling head's relation losses at the production shape (labnotes R17.4): L 9, B 2,
Q = R = 100, 133 classes, 56 predicates, 200 x 334 mask logits, 12 544 points, 20 relations per image.

  relation part alone          BaselineRelationLoss.loss(grads={}) on a finished segmentation matching
  full_losses / seg_losses     CrossHeadBaseline.full_losses against seg_losses alone
  the reference's way          the same three terms and gradients with torch ops on the device and
                               linear_sum_assignment(cost.cpu()) per image (what the reference executes)

HIP events around each call, warm-up first, median with min-max of `--iters` calls, `--repeats` times.

    python tools/rel_loss_probe.py [--iters 30] [--repeats 3] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
from scipy.optimize import linear_sum_assignment

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


def torch_way(rel, sub, obj, gt_rels, od, cw, B):
    """Steps 1-7 of the reference with torch ops on device tensors (fp32, autograd)."""
    rel, sub, obj = (t.detach().requires_grad_(True) for t in (rel, sub, obj))
    R = rel.shape[1]
    labels = torch.zeros(B, R, dtype=torch.long, device=rel.device)
    ls, lo = [], []
    for b in range(B):
        od_pos, gt_inds = od[b]
        a = torch.ones(len(gt_inds), dtype=torch.long, device=rel.device)
        a[gt_inds] = od_pos
        gr = gt_rels[b]
        gs, go = a[gr[:, 0]], a[gr[:, 1]]
        cost = -sub[b].softmax(-1)[:, gs] - obj[b].softmax(-1)[:, go] - rel[b].softmax(-1)[:, gr[:, 2]]
        r, c = linear_sum_assignment(cost.detach().cpu())
        r, c = torch.from_numpy(r).to(rel.device), torch.from_numpy(c).to(rel.device)
        labels[b, r] = gr[c, 2]
        ts = (od_pos[None, :] == gs[c][:, None]).nonzero()[:, 1]
        to = (od_pos[None, :] == go[c][:, None]).nonzero()[:, 1]
        fs, fo = sub[b][r][:, od_pos], obj[b][r][:, od_pos]
        ls.append(2.0 * torch.nn.functional.cross_entropy(fs, ts))
        lo.append(2.0 * torch.nn.functional.cross_entropy(fo, to))
    flat = labels.view(-1)
    ce = torch.nn.functional.cross_entropy(rel.view(B * R, -1), flat, weight=cw, reduction="none")
    total = 2.0 * ce.sum() / (cw[flat].sum() + torch.finfo(torch.float32).eps) + \
        torch.stack(ls).mean() + torch.stack(lo).mean()
    total.backward()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import baseline_loss_ref as BR
    from pairnet_amd import BaselineRelationLoss, CrossHeadBaseline, baseline_head_cfg
    case = BR.full_case(9, 2, 100, 133, 56, 200, 334, 12544, (23, 17), (20, 20), 41)
    cfg = baseline_head_cfg()
    cfg.pop("type")
    head = CrossHeadBaseline(**cfg)
    dev = lambda t: t.to(DEV).contiguous()
    cls = dict(cls=dev(case["cls"]), rel=dev(case["rel"]), subject_scores=dev(case["sub"]),
               object_scores=dev(case["obj"]))
    masks = dict(mask=dev(case["mask"]))
    metas = [dict()] * 2
    state = dict(step=0)

    def full():
        state["step"] += 1
        return head.full_losses(cls, masks, case["gt_rels"], None, case["gt_labels"], case["gt_masks"],
                                metas, grads={}, seed=1, step=state["step"])

    def seg():
        state["step"] += 1
        return head.seg_losses(cls, masks, case["gt_labels"], case["gt_masks"], metas, grads={},
                               seed=1, step=state["step"])

    full()
    torch.cuda.synchronize()
    assert int(head.seg_status().cpu()) == 0 and int(head.rel_status().cpu()) == 0
    matched = head._seg_loss.last["matched"].clone()
    rel_obj = BaselineRelationLoss(56, 100, 100)
    G = [23, 17]

    def rel_alone():
        return rel_obj.loss(cls["rel"], cls["subject_scores"], cls["object_scores"], case["gt_rels"],
                            matched, 2, grads={}, num_gts=G)

    od, _ = BR.od_of(matched.cpu(), 9, 2, case["gt_labels"])
    od_d = [(dev(q), dev(g)) for q, g in od]
    rels_d = [dev(g) for g in case["gt_rels"]]
    cw = torch.tensor(case["rel_class_weight"], device=DEV)

    def reference_way():
        return torch_way(cls["rel"], cls["subject_scores"], cls["object_scores"], rels_d, od_d, cw, 2)

    ours = rel_alone()
    want = reference_way()
    torch.cuda.synchronize()
    print("sum of the three terms: kernels %.6f, torch ops %.6f" % (float(sum(ours.values())), float(want)))
    res = dict(shape=dict(L=9, B=2, Q=100, R=100, Cr=56, Gr=20, h=200, w=334, Np=12544), runs=[])
    for rep in range(args.repeats):
        run = dict(relation_alone=timed(rel_alone, args.iters), seg_losses=timed(seg, args.iters),
                   full_losses=timed(full, args.iters), reference_way=timed(reference_way, args.iters))
        res["runs"].append(run)
        print(rep, {k: "%.3f ms (%.3f-%.3f)" % (v["median"], v["min"], v["max"]) for k, v in run.items()},
              flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
