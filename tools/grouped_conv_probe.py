"""Times pn_conv2d_grouped_nhwc_f32 (csrc/grouped_conv.hip) at the ResNeXt-101 32x8d shapes of one
800 x 1333 image -- the stride-1 blocks of the four stages and each stage's stride-2 first block --
beside two yardsticks on the same operands:

  (a) the only route without it: pn_conv2d_nhwc_ex_f32 on block-diagonally expanded dense weights
      (G times the multiplications);
  (b) torch.nn.functional.conv2d(groups=G) of PyTorch-ROCm on channels_last tensors.

Per row: microseconds (device events around `--iters` launches after a warm-up, the median of
`--repeats` windows, the three candidates alternating inside each repeat), TFLOP/s and GB/s from the
operations and bytes the shapes need (input + output + weights once), and the share of the nearer
roof: max(flops / 157.3 TF, bytes / 8 TB/s) over the time.  Then the whole ResNeXt-101 forward and
the detector's images/s at 800 x 1333 next to ResNet-101's (`--no-nets` skips them).

    python tools/grouped_conv_probe.py [--iters 50] [--repeats 5] [--no-nets]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12
DEV = "cuda:0"
# (name, H, W of the INPUT map, C, Cg, stride)
SHAPES = [
    ("stage 1        ", 200, 334, 256, 8, 1),
    ("stage 2        ", 100, 167, 512, 16, 1),
    ("stage 3        ", 50, 84, 1024, 32, 1),
    ("stage 4        ", 25, 42, 2048, 64, 1),
    ("stage 2 first/2", 200, 334, 512, 16, 2),
    ("stage 3 first/2", 100, 167, 1024, 32, 2),
    ("stage 4 first/2", 50, 84, 2048, 64, 2),
]


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1e3 * s.elapsed_time(e) / iters          # microseconds per call


def compare(fns, iters, repeats):
    """{name: median microseconds}; the candidates alternate inside every repeat."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def kernels(args):
    from pairnet_amd import hip
    hip.lib()
    g = torch.Generator().manual_seed(0)
    print("%-16s %-22s %9s %8s %8s %7s   [min .. max us]" % ("shape", "route", "us", "TFLOP/s", "GB/s",
                                                          "roof"))
    for name, H, W, C, Cg, s in SHAPES:
        G = C // Cg
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        x = torch.randn(1, H, W, C, generator=g).to(DEV)
        w = (torch.randn(C, Cg, 3, 3, generator=g) * (9 * Cg) ** -0.5).to(DEV)
        b = torch.randn(C, generator=g).to(DEV)
        wg = w.permute(0, 2, 3, 1).reshape(G, Cg, 9 * Cg).contiguous()
        dense = torch.zeros(C, 3, 3, C, device=DEV)          # block diagonal, (ky, kx, ci) rows
        for gi in range(G):
            sl = slice(gi * Cg, (gi + 1) * Cg)
            dense[sl, :, :, sl] = w[sl].permute(0, 2, 3, 1)
        dense = dense.reshape(C, 9 * C)
        out, out_a = torch.empty(1, Ho, Wo, C, device=DEV), torch.empty(1, Ho, Wo, C, device=DEV)
        scratch = torch.empty(16 * 1024 * 1024 // 2, device=DEV)
        x_cl = x.permute(0, 3, 1, 2)                          # NCHW-shaped, channels_last memory
        w_cl = w.contiguous(memory_format=torch.channels_last)
        fns = {
            "grouped kernel": lambda: hip.conv3x3_grouped(x, wg, b, out, 1, H, W, G, Cg, s, relu=True),
            "(a) dense conv2d_ex": lambda: hip.conv2d_ex(x, dense, b, None, out_a, 1, H, W, C, C, 3,
                                                         3, s, 1, relu=True, scratch=scratch),
            "(b) torch groups=": lambda: F.relu(F.conv2d(x_cl, w_cl, b, stride=s, padding=1,
                                                         groups=G)),
        }
        res = compare(fns, args.iters, args.repeats)
        # faster and different is not faster: the three agree to fp32 re-association
        y_b = fns["(b) torch groups="]().permute(0, 2, 3, 1)
        scale = float(y_b.abs().max())
        d_a, d_b = float((out - out_a).abs().max()) / scale, float((out - y_b).abs().max()) / scale
        flops = 2.0 * Ho * Wo * C * 9 * Cg
        nbytes = 4.0 * ((H * W + Ho * Wo) * C + C * 9 * Cg)
        floor = max(flops / PEAK_FLOPS, nbytes / PEAK_BYTES) * 1e6
        bound = "matrix pipe" if flops / PEAK_FLOPS > nbytes / PEAK_BYTES else "HBM"
        for k, (us, lo, hi) in res.items():
            print("%-16s %-22s %9.1f %8.2f %8.0f %6.1f%%   [%.1f .. %.1f]" % (
                name, k, us, flops / us * 1e-6, nbytes / us * 1e-3, 100.0 * floor / us, lo, hi),
                flush=True)
        print("%-16s floor %.1f us (%s); max |kernel - (a)| %.1e, |kernel - (b)| %.1e of the largest "
              "entry; kernel / (a) = %.3f, kernel / (b) = %.3f" % (
                  name, floor, bound, d_a, d_b, res["grouped kernel"][0] / res["(a) dense conv2d_ex"][0],
                  res["grouped kernel"][0] / res["(b) torch groups="][0]), flush=True)


def nets(args):
    import pairnet_amd as P
    img = torch.randn(1, 3, 800, 1333, generator=torch.Generator().manual_seed(1)).to(DEV)
    rx, rn = P.ResNeXtHip(101, 32, 8).to(DEV), P.ResNet50Hip(depth=101).to(DEV)
    fns = {"ResNeXt-101 32x8d forward": lambda: rx(img), "ResNet-101 forward": lambda: rn(img)}
    for k, (us, lo, hi) in compare(fns, max(args.iters // 5, 5), args.repeats).items():
        print("%-28s %9.2f ms   [%.2f .. %.2f]" % (k, us * 1e-3, lo * 1e-3, hi * 1e-3), flush=True)
    del rx, rn
    metas = [dict(batch_input_shape=(800, 1333), img_shape=(800, 1333, 3), scale_factor=[1.0] * 4)]
    dets = {"pairnet_rnext101_vg": P.build_detector(P.pairnet_rnext101_vg().model).to(DEV),
            "cross_r101_vg": P.build_detector(P.cross_r101_vg().model).to(DEV)}
    fns = {k: (lambda d=d: d.simple_test(img, metas, rescale=True)) for k, d in dets.items()}
    for k, (us, lo, hi) in compare(fns, max(args.iters // 5, 5), args.repeats).items():
        print("%-28s %9.2f images/s (simple_test, batch 1, host results; %.2f ms)" % (
            k, 1e6 / us, us * 1e-3), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-nets", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grouped_conv_probe.py measures on an MI355X; no GPU here")
    print(torch.cuda.get_device_name(0))
    kernels(args)
    if not args.no_nets:
        nets(args)


if __name__ == "__main__":
    main()
