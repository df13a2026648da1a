"""Times the no-graph-constraint box evaluation on the GPU (labnotes/r32.md).

    python tools/nogc_probe.py [--out FILE.json]

At R = 100 and C1 = 51 (VG) / 57 (PSG), all predicates kept (the reference's default threshold):
  * `pn_nogc_triplets_f32` beside its composition from what the library had before -- the
    products formed by torch (`(s_sub * s_obj)[:, None] * rel_dists[:, 1:]`), `pn_topk_f32` over
    them, and the gathers that turn the 100 indices into triplets and rows;
  * `StreamingEvaluator.add_boxes` with `nogc` off, on (default threshold), on with two
    thresholds, and on with `iou=True`.
Each figure is the median over BLOCKS windows of ITERS calls between two device events, after a
warm-up of every variant; the variants alternate window by window so that drift hits them alike.
The two rankings are compared before they are timed (the same 100 triplets).  Reads no file."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ITERS, BLOCKS, WARMUP, R, K = 200, 9, 20, 100, 100


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS                        # microseconds per call


def medians(variants):
    """{name: median us per call}, windows alternating over the variants."""
    for fn in variants.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(BLOCKS):
        for name, fn in variants.items():
            times[name].append(window(fn))
    return {name: dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)))
            for name, v in times.items()}


def case(C1, dev):
    from pairnet_amd import hip
    from pairnet_amd.evaluation import StreamingEvaluator
    rng = np.random.default_rng(C1)
    P1, n = C1 - 1, R * (C1 - 1)
    det = torch.from_numpy(np.concatenate(
        [rng.uniform(0, 400, (2 * R, 4)), rng.random((2 * R, 1))], 1).astype(np.float32)).to(dev)
    det[:, 2:4] += det[:, :2]
    labels = torch.from_numpy(rng.integers(1, 134, 2 * R)).to(dev)
    rel = torch.from_numpy(rng.random((R, C1)).astype(np.float32)).to(dev)
    ar = torch.arange(R, dtype=torch.int32, device=dev)
    i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
    i64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int64)
    trip, srow, orow, count = i32(K, 3), i32(K), i32(K), i32(1)
    score = torch.empty(K, device=dev, dtype=torch.float32)
    idx, quot, rem = i64(K), i64(K), i64(K)

    def fused():
        hip.nogc_triplets(det, 5, labels, rel, ar, ar + R, R, C1, P1, K, trip, srow, orow, score,
                          count)

    def composed():
        prod = ((det[:R, 4] * det[R:, 4])[:, None] * rel[:, 1:]).contiguous()
        hip.topk(prod, idx, quot, rem, 1, n, P1, K)
        t = torch.stack((labels[quot], rem + 1, labels[quot + R]), 1).to(torch.int32)
        return t, quot.to(torch.int32), (quot + R).to(torch.int32), prod.view(-1)[idx]

    fused()
    t2, s2, o2, sc2 = composed()
    torch.cuda.synchronize()
    same = bool(torch.equal(trip, t2) and torch.equal(srow, s2) and torch.equal(orow, o2)
                and torch.equal(score, sc2))
    out = dict(rank=medians(dict(fused=fused, composed=composed)), same_ranking=same)

    # add_boxes: one image with 10 ground-truth relations over 8 objects
    gt_boxes = np.concatenate([rng.uniform(0, 300, (8, 2)), rng.uniform(320, 400, (8, 2))], 1)
    gt_labels = rng.integers(1, 134, 8)
    gt_rels = np.array([[j % 8, (j + 1 + j // 8) % 8, 1 + j % P1] for j in range(10)])
    result = (det, labels, None, None, None, rel)
    evs = dict(plain=(StreamingEvaluator(P1), {}), nogc=(StreamingEvaluator(P1, nogc=True), {}),
               nogc_two=(StreamingEvaluator(P1, nogc=(3, P1)), {}),
               nogc_iou=(StreamingEvaluator(P1, nogc=True), dict(iou=True)))

    def adder(name):
        ev, kw = evs[name]

        def fn():
            ev.add_boxes(result, gt_rels, gt_labels, gt_boxes, **kw)
            if len(ev._dev) >= 64:                                # (records stay on the device;
                ev._dev.clear()                                   # dropped, never read back)
        return fn

    out["add_boxes"] = medians({name: adder(name) for name in evs})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the GPU"
    dev = torch.device("cuda:0")
    res = dict(R=R, K=K, iters=ITERS, blocks=BLOCKS,
               cases={"C1=%d" % C1: case(C1, dev) for C1 in (51, 57)})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
