"""Times the matching stage of PSGTrHead2's loss in two forms at the production shape (B 2, Q 100,
C 133, Cr 56, 200 x 334 logits, 400 x 668 masks, Np 12 544, (15, 14) objects, (30, 29) relations):

  new       `pn_tri_match_cost_f32` (csrc/tri_loss.hip): five launches for the batch, mask work per
            (side, query, OBJECT)
  composed  the same cost blocks per image from the entries that were there before:
            `pn_point_sample_f32` on both mask stacks and the ground truth, a gather of the
            ground-truth samples per RELATION, `pn_mask_match_cost_f32` per side (class + mask + dice)
            and `pn_id_match_cost_f32` for the predicate term, summed with torch adds

HIP events, warmed up, the two forms alternating inside one loop.  Also times the whole `loss` call
with and without `grads`, and -- for the record, the loss does not do it -- the copy of the two mask
stacks behind one base pointer.  Prints one JSON line; sets no threshold.

    python tools/tri_loss_probe.py [--iters 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import tri_loss_ref as T
    from pairnet_amd import PSGTrHead2Loss, hip
    dev = "cuda:0"
    case = T.tri_case(**T.PRODUCTION)
    B, Q = case["sub"].shape[1:3]
    D = lambda t: t.to(dev).contiguous()
    sub, obj, rel = (D(case[k][0]) for k in ("sub", "obj", "rel"))
    s_seg, o_seg = D(case["sub_seg"][0]), D(case["obj_seg"][0])
    gm = [D(m) for m in case["gt_masks"]]
    gl = [D(g.long()) for g in case["gt_labels"]]
    gr = [D(g.long()) for g in case["gt_rels"]]
    R, G = [g.shape[0] for g in gr], [g.shape[0] for g in gl]
    Np = case["num_points"]
    pts = torch.rand(B, Np, 2, generator=torch.Generator().manual_seed(1)).to(dev)
    tab, c, coffs = [], 0, []
    for b in range(B):
        coffs.append(c)
        tab += [c, R[b], sum(R[:b]), sum(G[:b]), G[b], sum(min(Q, r) for r in R[:b]), 0, 0]
        c += Q * R[b]
    tab = D(torch.tensor(tab).view(B, 8))
    gm_all, gl_all, gr_all = torch.cat(gm), torch.cat(gl), torch.cat(gr)
    w = list(T.CFG["cost"]) + list(T.CFG["cost_eps"])
    cost_new = torch.empty(c, device=dev)
    f32 = lambda *s: torch.empty(*s, device=dev)
    scratch = hip.tri_match_cost_scratch(B, Q, sum(G), Np, dev)

    def new():
        hip.tri_match_cost(sub, obj, rel, s_seg, o_seg, gm_all, pts, gr_all, gl_all, tab, w, max(G),
                           Q * max(R), cost_new, scratch)

    xs, xo = f32(Q, Np), f32(Q, Np)
    tb = [f32(G[b], Np) for b in range(B)]
    parts = [[f32(Q, R[b]) for _ in range(3)] for b in range(B)]
    cost_old = [f32(Q, R[b]) for b in range(B)]

    def composed():
        for b in range(B):
            hip.point_sample(s_seg[b], pts[b], xs)
            hip.point_sample(o_seg[b], pts[b], xo)
            hip.point_sample(gm[b], pts[b], tb[b])
            so, oo, pr = gr[b][:, 0], gr[b][:, 1], gr[b][:, 2].contiguous()
            ls, lo = gl[b][so], gl[b][oo]
            hip.mask_match_cost(sub[b], ls, xs, tb[b][so].contiguous(), parts[b][0], w[0], w[1], w[2], w[7])
            hip.mask_match_cost(obj[b], lo, xo, tb[b][oo].contiguous(), parts[b][1], w[3], w[4], w[5], w[8])
            hip.id_match_cost(sub[b], obj[b], rel[b], ls, lo, pr, parts[b][2], 0.0, 0.0, w[6])
            torch.add(parts[b][0], parts[b][1], out=cost_old[b])
            cost_old[b] += parts[b][2]

    loss_obj = PSGTrHead2Loss(case["num_classes"], case["num_relations"], Q)
    cls_d = dict(sub=sub[None], obj=obj[None], rel=rel[None])
    seg_d = dict(sub_seg=s_seg[None], obj_seg=o_seg[None])

    def loss(grads):
        loss_obj.loss(cls_d, seg_d, case["gt_rels"], None, case["gt_labels"], gm, [dict()] * B,
                      grads={} if grads else None, seed=1, step=1)

    stacked = f32(2, B, Q, *s_seg.shape[-2:])

    def copy():
        stacked[0].copy_(s_seg)
        stacked[1].copy_(o_seg)

    forms = dict(new=new, composed=composed, loss_values=lambda: loss(False),
                 loss_with_grads=lambda: loss(True), stack_copy=copy)
    for fn in forms.values():             # warm-up: every form three times
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(args.iters):           # alternating: one of each per round
        for k, fn in forms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    # the two forms compute the same blocks (different summation orders: a few roundings apart)
    diff = max(float((cost_new[coffs[b]:coffs[b] + Q * R[b]].view(Q, R[b]) - cost_old[b]).abs().max())
               for b in range(B))
    out = dict(shape=dict(B=B, Q=Q, Np=Np, G=G, R=R), iters=args.iters, max_abs_diff_new_vs_composed=diff)
    for k, v in ms.items():
        v = np.asarray(v)
        out[k] = dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4),
                      max_ms=round(float(v.max()), 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
