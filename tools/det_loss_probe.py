"""What the plain detector's loss costs on one MI355X (pair-net_amd/det_losses.py, csrc/det_loss.hip)
at the config's shapes: B 4, 1024 x 1024 (21 760 encoder tokens), C 150, L 6, Q 100
(od_r101_vg.py) and Q 300 (od_rnext101_vg.py), 12 boxes per image, on synthetic head outputs.

Per query count: ms per `DeformableDETRLoss.loss` call (device wait at both ends), each kernel
alone (HIP events around repeated launches on the call's own operands), the host-mode assignment's
share (cost download + scipy), and beside them the same terms composed from torch ops on the GPU
(focal term of the concatenated rows with its gradient by autograd; L1 + GIoU of the matched pairs
with theirs; the cost blocks by broadcasting).

    python tools/det_loss_probe.py [reps] [--out profiles/det_loss.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

from pairnet_amd import DeformableDETRLoss, det_train_cfg, hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
L, B, C, G, SIDE = 6, 4, 150, 12, 1024
SN = sum(((SIDE // s) ** 2) for s in (8, 16, 32, 64))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def boxes(g, *lead):
    return torch.cat([torch.rand(*lead, 2, generator=g) * 0.7 + 0.15,
                      torch.rand(*lead, 2, generator=g) * 0.25 + 0.03], -1)


def focal_torch(x, labels, avg_rows, alpha=0.25, gamma=2.0, w=2.0):
    """mmdet's py_sigmoid_focal_loss on the concatenated rows, per-row 1 / avg, and its gradient."""
    x = x.detach().requires_grad_(True)
    t = F.one_hot(labels.long(), C + 1)[:, :C].to(x.dtype)
    p = x.sigmoid()
    pt = (1 - p) * t + p * (1 - t)
    fw = (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)
    loss = (F.binary_cross_entropy_with_logits(x, t, reduction="none") * fw).sum(-1)
    total = (w * loss / avg_rows).sum()
    total.backward()
    return total, x.grad


def box_torch(pred, gt, f, avg):
    import det_loss_ref as R
    pred = pred.detach().requires_grad_(True)
    l1, gi = R.box_terms(pred, gt, f)
    total = 5.0 * l1 / avg + 2.0 * gi / avg
    total.backward()
    return total, pred.grad


def cost_torch(cls, box, gl, gt, f):
    import det_loss_ref as R
    return R.match_cost(cls, box, gl, gt, f, dtype=torch.float32)


out = {"what": "DeformableDETRLoss.loss at B %d, %d x %d (SN %d), C %d, L %d, %d boxes per image; ms"
               % (B, SIDE, SIDE, SN, C, L, G), "reps": args.reps}
for Q in (100, 300):
    g = torch.Generator().manual_seed(Q)
    cls = (torch.randn(L, B, Q, C, generator=g) * 2 - 2).to(dev)
    enc_cls = (torch.randn(B, SN, C, generator=g) * 2 - 2).to(dev)
    box, enc_box = boxes(g, L, B, Q).to(dev), boxes(g, B, SN).to(dev)
    metas = [dict(img_shape=(SIDE, SIDE, 3))] * B
    f4 = torch.tensor([SIDE] * 4, dtype=torch.float32)
    gtb, gtl = [], []
    for _ in range(B):
        c, s = torch.rand(G, 2, generator=g) * 0.6 + 0.2, torch.rand(G, 2, generator=g) * 0.3 + 0.05
        gtb.append(torch.cat([c - s / 2, c + s / 2], -1) * f4)
        gtl.append(torch.randint(0, C, (G,), generator=g))
    lo = DeformableDETRLoss(C, train_cfg=det_train_cfg())
    call = lambda: lo.loss(cls, box, enc_cls, enc_box, gtb, gtl, metas, grads={})
    r = {"loss_call": wall(call, args.reps)}
    # ---- each kernel alone on the call's operands ----
    n_dec, rows, T = L * B * Q, L * B * Q + B * SN, L + 1
    X = torch.cat([cls.reshape(n_dec, C), enc_cls.reshape(B * SN, C)])
    PB = torch.cat([box.reshape(n_dec, 4), enc_box.reshape(B * SN, 4)])
    r["concat_rows"] = timed(lambda: (torch.cat([cls.reshape(n_dec, C), enc_cls.reshape(B * SN, C)]),
                                      torch.cat([box.reshape(n_dec, 4), enc_box.reshape(B * SN, 4)])),
                             args.reps)
    trace = []
    lo.loss(cls, box, enc_cls, enc_box, gtb, gtl, metas, trace=trace)
    tab, c_off, probs = [], 0, []
    for t in range(T):
        n = Q if t < L else SN
        for b in range(B):
            roff = (t * B + b) * Q if t < L else n_dec + b * SN
            tab += [c_off, n, G, b * G + (B * G if t == L else 0), b * G, roff]
            probs.append((n, c_off))
            c_off += n * G
    tab = torch.tensor(tab, dtype=torch.int64, device=dev).view(-1, 6)
    labs = torch.cat(gtl + [torch.zeros(B * G, dtype=torch.int64)]).to(dev)
    gt_dev = torch.cat(gtb).to(dev)
    pfac = f4.view(1, 4).expand(len(probs), 4).contiguous().to(dev)
    cost = torch.empty(c_off, device=dev)
    r["pn_det_match_cost_f32"] = timed(lambda: hip.det_match_cost(
        X, PB, labs, gt_dev, pfac, tab, cost, SN * G), args.reps)
    t0 = time.perf_counter()
    for _ in range(args.reps):
        host = cost.cpu().numpy()
        for n, co in probs:
            linear_sum_assignment(host[co:co + n * G].reshape(n, G))
    r["host_assignment"] = (time.perf_counter() - t0) * 1e3 / args.reps
    labels = torch.full((rows,), C, device=dev, dtype=torch.int32)
    pairs = []
    for e in trace:
        t, b = e["term"], e["image"]
        roff = (t * B + b) * Q if t < L else n_dec + b * SN
        rr = torch.from_numpy(e["rows"]) + roff
        labels[rr.to(dev)] = (torch.zeros(len(rr), dtype=torch.int32) if t == L
                              else gtl[b][torch.from_numpy(e["cols"])].to(torch.int32)).to(dev)
        pairs.append(np.stack([rr.numpy(), e["cols"] + b * G, np.full(len(rr), b), np.full(len(rr), t)], 1))
    pairs = torch.from_numpy(np.concatenate(pairs).astype(np.int32)).to(dev)
    M = pairs.shape[0]
    counts = [int((pairs[:, 3] == t).sum()) for t in range(T)]
    toff = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=dev)
    avg = torch.tensor([float(max(c_, 1)) for c_ in counts], device=dev)
    term = lo._term_ids(L, B, Q, SN, dev)
    gX, gB = torch.empty(rows, C, device=dev), torch.zeros(rows, 4, device=dev)
    part = torch.empty(hip.det_focal_partials(rows, C, T), device=dev)
    oc, ob = torch.empty(T, device=dev), torch.empty(T, 2, device=dev)
    r["pn_det_focal_f32"] = timed(lambda: hip.det_focal(X, labels, term, avg, gX, part, oc), args.reps)
    r["pn_det_focal_f32_GBps"] = 2 * rows * C * 4 / (r["pn_det_focal_f32"] * 1e-3) / 1e9
    fac = f4.view(1, 4).expand(B, 4).contiguous().to(dev)
    r["pn_det_box_loss_f32"] = timed(lambda: hip.det_box_loss(PB, gt_dev, fac, pairs, toff, avg, gB, ob),
                                     args.reps)
    r["matched_pairs"] = M
    # ---- the same terms from torch ops on the GPU ----
    avg_rows = avg[term.long()]
    r["torch_focal_fwd_bwd"] = timed(lambda: focal_torch(X, labels, avg_rows), args.reps)
    pr, pg = pairs[:, 0].long(), pairs[:, 1].long()
    fM = f4.view(1, 4).expand(M, 4).to(dev)
    r["torch_box_fwd_bwd"] = timed(lambda: box_torch(PB[pr], gt_dev[pg], fM, avg[pairs[:, 3].long()].mean()),
                                   args.reps)
    fd, tab_h = f4.to(dev), tab.tolist()
    r["torch_cost"] = timed(lambda: [cost_torch(X[ro:ro + n], PB[ro:ro + n], labs[lo_:lo_ + G],
                                                gt_dev[bo:bo + G], fd)
                                     for (_, n, _, lo_, bo, ro) in tab_h], args.reps)
    out["Q%d" % Q] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
