"""Stand-alone timing of the result-mask step at the 800 x 1333 shape (Q = R = 100,
200 x 334 -> 384 x 640): the launch sequence of rounds 1-11 (two pn_gather_rows_f32 of the
mask logits + two pn_bilinear_planar_gt0_u8) against pn_pair_masks_u8, HIP events around
every call, on three index sets -- the pairs a real forward selects (seeded weights and
features as bench.py --path head builds them), 100 distinct objects, one object for all
slots -- with the streaming rate of k_s3_split measured in the same process beside them,
and pn_resize_kept_f32's two forms for nkeep = 1, 10, 100.

    python tools/pair_masks_probe.py [--calls 60] [--json OUT]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"


def events_us(fn, calls, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(calls)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    t = sorted(s.elapsed_time(e) * 1e3 for s, e in ev)
    return dict(min=t[0], median=t[len(t) // 2], p90=t[int(len(t) * 0.9)], max=t[-1])


def real_indices():
    from pairnet_amd import CrossHead2, pairnet_head_cfg
    cfg = pairnet_head_cfg()
    cfg.pop("type")
    head = CrossHead2(**cfg)
    head.init_weights(seed=0)
    head.to(DEV)
    g = torch.Generator().manual_seed(1000)
    H, W = 800, 1333
    shapes, h, w = [], (H + 1) // 2, (W + 1) // 2
    for _ in range(4):                      # strides 4, 8, 16, 32
        h, w = (h + 1) // 2, (w + 1) // 2
        shapes.append((h, w))
    feats = [torch.relu(torch.randn(1, c, h, w, generator=g)).to(DEV)
             for c, (h, w) in zip((256, 512, 1024, 2048), shapes)]
    sf = 2.083
    _, masks = head.forward(feats, [dict(img_shape=(H, W, 3), scale_factor=[sf] * 4)])
    torch.cuda.synchronize()
    sub, obj = head.pair_positions()
    return sub[0].clone(), obj[0].clone(), masks["mask"][0].reshape(100, -1).clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from pairnet_amd import hip
    Q = R = 100
    hi, wi, ho, wo = 200, 334, 384, 640
    sub_r, obj_r, mp = real_indices()
    assert mp.shape == (Q, hi * wi), mp.shape
    perm = torch.randperm(Q, generator=torch.Generator().manual_seed(2)).to(DEV)
    sets = {"real": (sub_r, obj_r),
            "distinct100": (torch.arange(Q, device=DEV), perm),
            "one_object": (torch.full((R,), 17, device=DEV), torch.full((R,), 17, device=DEV))}
    seg = torch.empty(2 * R, hi * wi, device=DEV)
    want = torch.empty(2 * R, ho, wo, device=DEV, dtype=torch.uint8)
    got = torch.empty_like(want)
    out = {"shape": [Q, R, hi, wi, ho, wo], "calls": args.calls, "sets": {}}
    mb = (Q * hi * wi * 4 + 2 * R * ho * wo) / 1e6          # each logit row once + the masks

    for name, (sub, obj) in sets.items():
        def old():
            hip.gather_rows(mp, sub, seg[:R], 1, Q, R, hi * wi)
            hip.gather_rows(mp, obj, seg[R:], 1, Q, R, hi * wi)
            hip.bilinear_planar_gt0(seg[:R], want[:R], R, hi, wi, ho, wo)
            hip.bilinear_planar_gt0(seg[R:], want[R:], R, hi, wi, ho, wo)

        def new():
            hip.pair_masks(mp, sub, obj, got, Q, R, hi, wi, ho, wo)
        a, b = events_us(old, args.calls), events_us(new, args.calls)
        assert torch.equal(want, got), name
        distinct = len(set(sub.tolist()) | set(obj.tolist()))
        out["sets"][name] = dict(distinct_objects=distinct, sequence_us=a, pair_masks_us=b, MB=mb,
                                 pair_masks_GBps=mb * 1e3 / b["median"])
        print("%-12s %3d objects: sequence %7.1f us (min %.1f max %.1f)   pair_masks %6.1f us "
              "(min %.1f max %.1f)  %.0f GB/s on %.0f MB" % (
                  name, distinct, a["median"], a["min"], a["max"], b["median"], b["min"], b["max"],
                  mb * 1e3 / b["median"], mb), flush=True)

    # the streaming yardstick: k_s3_split reads 4 and writes 6 bytes per element
    rows, K = 26720, 1024
    x = torch.randn(rows, K, device=DEV)
    s3 = torch.empty(hip.s3_floats(rows, K), device=DEV)
    t = events_us(lambda: hip.s3_split(x, s3), args.calls)
    out["k_s3_split"] = dict(us=t, MB=10.0 * rows * K / 1e6, GBps=10.0 * rows * K / 1e3 / t["median"])
    print("k_s3_split   %.0f MB: %.1f us  %.0f GB/s" % (out["k_s3_split"]["MB"], t["median"],
                                                       out["k_s3_split"]["GBps"]), flush=True)

    out["resize_kept"] = {}
    up = torch.empty(Q, ho * wo, device=DEV)
    for nkeep in (1, 10, 100):
        st = torch.zeros(hip.panoptic_state_bytes() // 4, dtype=torch.int32)
        st[0] = nkeep
        st[16:16 + nkeep] = torch.arange(nkeep, dtype=torch.int32)
        st = st.to(DEV).view(torch.uint8)
        r = {}
        for form in (0, 1):
            r["form%d_us" % form] = events_us(
                lambda: hip.resize_kept(mp, up, st, Q, hi, wi, ho, wo, form=form), args.calls)
        out["resize_kept"][str(nkeep)] = r
        print("resize_kept  nkeep %3d: blocks %.1f us   strips %.1f us" % (
            nkeep, r["form0_us"]["median"], r["form1_us"]["median"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
