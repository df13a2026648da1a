"""What evaluating costs inside `dist.multi_gpu_test` (one rank): images/s of the loop

  none    no evaluator (the loop `bench.py`'s multi_gpu_test_product_loop leg times),
  host    `TripletEvaluator` + `SceneGraphMetrics`: about ten blocking copies per image,
  stream  `StreamingEvaluator`: records stay on the device until the end of the pass,

on the R50 detector with seeded weights.  The ground truth is cut on the device from a warm-up
pass's own results (the first `--rels` triplets of each image: their masks, labels and
predicates), so matches exist.  Every variant is warmed up once, then the variants alternate for
`--passes` passes; the host and the streaming metrics must be equal.

    python tools/eval_loop_probe.py [--package ROOT] [--images 240] [--passes 3] [--out FILE]

`--package ROOT`: the checkout whose `pairnet_amd` (and built library) to import -- the probe
run from this tree against a checkout of the previous commit gives that commit's `none` and
`host` rates in the same session (a tree without `StreamingEvaluator` skips `stream`).
Prints one JSON line; `--out` also writes it to a file."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--images", type=int, default=240)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--pool", type=int, default=8, help="distinct images (cycled)")
    ap.add_argument("--rels", type=int, default=10, help="ground-truth relations per image")
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--variants", default="none,host,stream")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import numpy as np
    import torch
    from oracle.backbone import seeded_backbone_state      # (seeded weights only)
    import pairnet_amd
    from pairnet_amd import build_detector, pairnet_r50
    from pairnet_amd.dist import multi_gpu_test
    from pairnet_amd.evaluation import SceneGraphMetrics, TripletEvaluator
    pkg_root = os.path.dirname(os.path.dirname(os.path.abspath(pairnet_amd.__file__)))
    assert pkg_root == os.path.abspath(args.package), (pkg_root, args.package)
    variants = [v for v in args.variants.split(",") if v]
    if "stream" in variants and not hasattr(pairnet_amd.evaluation, "StreamingEvaluator"):
        variants.remove("stream")

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    det = build_detector(pairnet_r50())
    det.backbone.load_state_dict(seeded_backbone_state(41))
    det.bbox_head.init_weights(seed=3)
    det.to(dev)
    H, W, N = args.height, args.width, args.images
    metas = [dict(img_shape=(H, W, 3), scale_factor=[2.083] * 4)]
    g = torch.Generator(device=dev).manual_seed(7)
    pool = [torch.randn(1, 3, H, W, generator=g, device=dev) for _ in range(args.pool)]
    head, R = det.bbox_head, det.bbox_head.num_rel_query
    n_rel = min(args.rels, R)
    rows = [r + o for r in range(n_rel) for o in (0, R)]     # subject, object of triplet r
    pool_ann = []
    for img in pool:                                          # the warm-up pass: its own results
        res = head.simple_test(det.extract_feat(img), metas)[0]
        pred = 1 + res[7][:n_rel, 1:].argmax(1).cpu().numpy()
        rels = np.array([[2 * j, 2 * j + 1, int(pred[j])] for j in range(n_rel)])
        pool_ann.append(dict(gt_rels=rels, gt_labels=res[1][rows].cpu().numpy(),
                             gt_masks=res[3][rows].clone()))
    torch.cuda.synchronize()
    data = [(pool[i % len(pool)], metas) for i in range(N)]
    ann = [pool_ann[i % len(pool)] for i in range(N)]

    def run(variant):
        kw = dict(depth=args.depth)
        if variant == "host":
            kw.update(annotations=ann, evaluator=TripletEvaluator(), metrics=SceneGraphMetrics(56))
        elif variant == "stream":
            kw.update(annotations=ann, evaluator=pairnet_amd.evaluation.StreamingEvaluator(56))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = multi_gpu_test(det, data, **kw)
        torch.cuda.synchronize()
        return N / (time.perf_counter() - t0), out.get("metrics")

    rates, metrics = {v: [] for v in variants}, {}
    for v in variants:                                        # warm-up (plans, calibration)
        run(v)
    for _ in range(args.passes):
        for v in variants:
            r, m = run(v)
            rates[v].append(round(r, 2))
            metrics[v] = m
    equal = None
    if "host" in metrics and "stream" in metrics:
        equal = metrics["host"] == metrics["stream"]
        assert equal, "the streaming metrics differ from the host path's"
    m = metrics.get("stream") or metrics.get("host")
    rec = dict(package=os.path.abspath(args.package), images=N, passes=args.passes,
               size=[H, W], mask_size=list(pool_ann[0]["gt_masks"].shape[-2:]),
               relations_per_image=n_rel, depth=args.depth, images_per_s=rates,
               spread={v: round(max(r) - min(r), 2) for v, r in rates.items()},
               metrics_equal=equal,
               metrics=None if m is None else {k: m[k] for k in (
                   "images", "skipped", "sgdet_recall", "phrdet_recall", "sgdet_mean_recall")})
    line = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
