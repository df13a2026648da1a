"""What `TrainPipeline.batch` costs on one MI355X at the production shapes, next to the same work
done stage by stage with the kernels the project had before csrc/augment.hip.

Two 480 x 640 images with G = 20 segments each: image 0 under policy 1 at (800, 1333) -> 800 x 1067,
image 1 under policy 2 (Resize (600, 1333) -> 600 x 800, a 480 x 560 window, Resize (800, 1333) ->
800 x 933), flipped.  The staged path: `hip.pan_masks` at PNG size, torch flip, torch index gathers
for the two nearest resizes and the crop, `hip.gt_mask_prepare`; `hip.preprocess_u8` for the image
(for policy 2 it resizes the source once to the final size: the project had no uint8 resize, so
that image is NOT the pipeline's result -- same traffic, other values; the masks of both paths are
compared and must be equal).  Its index tensors are built once, outside the timed window.

Both paths are timed in this process, warm, alternating, with device events over windows of
> 100 ms; the three new kernels are also timed alone against the bytes their shapes say they move.
Writes one JSON record (default profiles/train_pipeline.json).  Reports; gates nothing.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pairnet_amd import AugParams, TrainPipeline, hip, train_pipeline_cfg  # noqa: E402
from pairnet_amd.train_pipeline import cv_nearest_index  # noqa: E402

HBM_GBS = 8000.0        # MI355X HBM3E peak, GB/s


def sample(seed, H=480, W=640, rows=4, cols=5):
    """A decoded image, a panoptic PNG of rows x cols block segments, and their annotation."""
    rng = np.random.RandomState(seed)
    G = rows * cols
    ids = rng.choice(np.arange(1, 2 ** 24 - 1), G, replace=False).astype(np.int64)
    gy, gx = np.arange(H) * rows // H, np.arange(W) * cols // W
    seg = ids[gy[:, None] * cols + gx[None, :]]
    pan = np.stack([seg % 256, (seg // 256) % 256, seg // 65536], -1).astype(np.uint8)
    boxes = np.array([[c * W / cols, r * H / rows, (c + 1) * W / cols, (r + 1) * H / rows]
                      for r in range(rows) for c in range(cols)], dtype=np.float32)
    rels = np.array([[g, g + 1, 1 + g % 56] for g in range(G - 1)], dtype=np.int32)
    ann = dict(bboxes=boxes, labels=rng.randint(0, 133, G).astype(np.int64), rels=rels,
               masks=[dict(id=int(i), category=0, is_thing=1) for i in ids])
    return rng.randint(0, 256, (H, W, 3)).astype(np.uint8), pan, ann


def timed(fn, min_ms=120.0):
    """ms per call of `fn` over a window of at least `min_ms` (device events, warm)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n = 8
    while True:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        e.synchronize()
        ms = s.elapsed_time(e)
        if ms >= min_ms:
            return ms / n
        n *= 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "train_pipeline.json"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_pipeline_probe needs the MI355X; nothing is measured without it")
    dev = torch.device("cuda:0")
    pipe = TrainPipeline.from_config(train_pipeline_cfg(), device=dev)
    host = [sample(1), sample(2)]
    samples = [(torch.from_numpy(i).to(dev), torch.from_numpy(p).to(dev), a) for i, p, a in host]
    params = [AugParams(False, 0, (800, 1333), None, None),
              AugParams(True, 1, (600, 1333), (480, 560, 60, 120), (800, 1333))]
    geo = [pipe.geometry(480, 640, p) for p in params]
    tgt = [pipe.targets(s[2], p, g) for s, p, g in zip(samples, params, geo)]
    assert all(t is not None for t in tgt)
    Hb, Wb = max(g["pad"][0] for g in geo), max(g["pad"][1] for g in geo)
    fused = lambda: pipe.batch(samples, slot=0, params=params)

    # ---- the staged path, with what the project had before ----
    idx = lambda a: torch.from_numpy(a).to(dev)
    st = []
    for (img, pan, ann), p, g, t in zip(samples, params, geo, tgt):
        (H1, W1), (oy, ox, ch, cw), (H2, W2) = g["size1"], g["window"], g["size2"]
        G = len(ann["masks"])
        st.append(dict(
            ids=torch.tensor([m["id"] for m in ann["masks"]], dtype=torch.int32, device=dev),
            full=torch.empty((G, 480, 640), dtype=torch.uint8, device=dev),
            keep=idx(t["keep"]), y1=idx(cv_nearest_index(H1, 480)), x1=idx(cv_nearest_index(W1, 640)),
            y2=idx(cv_nearest_index(H2, ch)), x2=idx(cv_nearest_index(W2, cw)),
            out=torch.empty((len(t["keep"]), Hb // 2, Wb // 2), dtype=torch.uint8, device=dev)))
    img_out = torch.empty((2, 3, Hb, Wb), dtype=torch.float32, device=dev)

    def staged():
        for i, ((img, pan, ann), p, g, s) in enumerate(zip(samples, params, geo, st)):
            (H1, W1), (oy, ox, ch, cw), (H2, W2) = g["size1"], g["window"], g["size2"]
            hip.pan_masks(pan, s["ids"], None, s["full"])
            m = s["full"].flip(2) if p.flip else s["full"]
            m = m.index_select(1, s["y1"]).index_select(2, s["x1"])
            if p.crop is not None:
                m = m.index_select(0, s["keep"])[:, oy:oy + ch, ox:ox + cw]
                m = m.index_select(1, s["y2"]).index_select(2, s["x2"])
            hip.gt_mask_prepare(m.contiguous(), s["out"], Hb, Wb)
            src = img.flip(1).contiguous() if p.flip else img
            hip.preprocess_u8(src, 480, 640, img_out[i], H2, W2, Hb, Wb, pipe._mean[0],
                              pipe._mean[1], True)

    got = fused()
    staged()
    torch.cuda.synchronize()
    assert all(torch.equal(a.masks, s["out"]) for a, s in zip(got["gt_masks"], st)), \
        "the fused and the staged masks differ"
    assert torch.equal(got["img"][0], img_out[0])
    a, b = [], []
    for _ in range(args.rounds):                    # alternating, so that drift hits both alike
        a.append(timed(fused))
        b.append(timed(staged))

    # ---- the new kernels alone, against the bytes their shapes move ----
    kernels = {}

    def kernel(name, fn, nbytes):
        ms = statistics.median(timed(fn) for _ in range(3))
        kernels[name] = dict(us=round(1e3 * ms, 2), bytes=int(nbytes),
                             gb_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1),
                             share_of_hbm_peak=round(nbytes / (ms * 1e-3) / 1e9 / HBM_GBS, 4))
    for i, ((img, pan, ann), p, g, t) in enumerate(zip(samples, params, geo, tgt)):
        (H1, W1), (oy, ox, ch, cw), (H2, W2) = g["size1"], g["window"], g["size2"]
        Gk = len(t["keep"])
        ids = st[i]["ids"].index_select(0, st[i]["keep"].to(torch.int64)).contiguous()
        out = torch.empty((Gk, Hb // 2, Wb // 2), dtype=torch.uint8, device=dev)
        # PNG read once (an upper bound: the half-size map skips rows and columns) + masks written
        kernel("k_augment_masks[policy %d, Gk=%d]" % (p.policy + 1, Gk),
               lambda: hip.augment_masks(pan, ids, p.flip, (H1, W1), g["window"], (H2, W2),
                                         (Hb, Wb), out),
               480 * 640 * 3 + Gk * (Hb // 2) * (Wb // 2))
        src, sh, sw = img, 480, 640
        if p.crop is not None:
            win = torch.empty((ch, cw, 3), dtype=torch.uint8, device=dev)
            kernel("k_augment_resize_crop[%dx%d]" % (ch, cw),
                   lambda: hip.augment_resize_crop(img, 480, 640, p.flip, H1, W1, oy, ox, win),
                   480 * 640 * 3 + ch * cw * 3)
            src, sh, sw = win, ch, cw
        kernel("k_augment_image[policy %d]" % (p.policy + 1),
               lambda: hip.augment_image(src, sh, sw, p.flip and p.crop is None, img_out, i, H2,
                                         W2, pipe._mean[0], pipe._mean[1], True),
               sh * sw * 3 + 3 * Hb * Wb * 4)

    # bytes the mask stages write + read, stage by stage, against the fused kernel's
    staged_mask_bytes = 0
    for g, t, (img, pan, ann) in zip(geo, tgt, samples):
        (H1, W1), (oy, ox, ch, cw), (H2, W2) = g["size1"], g["window"], g["size2"]
        G, Gk = len(ann["masks"]), len(t["keep"])
        sizes = [G * 480 * 640, G * H1 * W1] + ([Gk * ch * cw, Gk * H2 * W2] if (ch, cw) != (H1, W1)
                                                else []) + [Gk * (Hb // 2) * (Wb // 2)]
        staged_mask_bytes += 480 * 640 * 3 + sizes[0] + sum(x + y for x, y in zip(sizes, sizes[1:]))
    fused_mask_bytes = sum(v["bytes"] for k, v in kernels.items() if "masks" in k)
    rec = dict(
        what="TrainPipeline.batch, two 480x640 images, G=20, policy 1 -> 800x1067 and policy 2 "
             "(flip, 600x800, window 480x560, -> 800x933), batch tensor %dx%d" % (Hb, Wb),
        device=torch.cuda.get_device_name(0),
        us_per_batch_fused=round(1e3 * statistics.median(a), 1),
        us_per_batch_staged=round(1e3 * statistics.median(b), 1),
        us_per_batch_fused_rounds=[round(1e3 * v, 1) for v in a],
        us_per_batch_staged_rounds=[round(1e3 * v, 1) for v in b],
        staged_over_fused=round(statistics.median(b) / statistics.median(a), 2),
        launches_fused=sum(2 if p.crop is None else 3 for p in params) + 1,
        mask_bytes_staged=int(staged_mask_bytes), mask_bytes_fused=int(fused_mask_bytes),
        mask_traffic_ratio=round(staged_mask_bytes / fused_mask_bytes, 1),
        kernels=kernels, hbm_peak_gb_per_s=HBM_GBS,
        note="times include the host side of each path (geometry, boxes, launches); the staged "
             "path's policy-2 image is one resize of the source, not the pipeline's result")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
