"""pn_msda_bwd_f32 (float atomics) against pn_msda_bwd_det_f32 (inverted index, no float atomics;
csrc/msda_grad.hip) at the 800 x 1333 encoder shape: N = Nq = 21 950, L = 3, B = 1 and 2, with the
layer's initial offsets and with init + N(0, 8 px) offsets (the two inputs of tools/msda_ab.py).
The two entries are timed ALTERNATELY with HIP events after a warm-up; median and spread (min ..
max) over the alternations.  Then `TailTrainer` scope "all" (ResNet-50 stages 2-4 + head, from the
image; the tests' 96 x 128 batch of two, or --train-hw 800,1333 for one image of that size) with
the switch off and on, alternately.  JSON lines.

    python tools/msda_bwd_det_probe.py [--reps 5] [--iters 20] [--no-trainer] [--no-kernels]
                                       [--train-hw 96,128] [--out FILE]

The per-kernel split of the deterministic entry comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/msda_bwd_det_probe.py --no-trainer`."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
SHAPES = [(25, 42), (50, 84), (100, 167)]
SN = sum(h * w for h, w in SHAPES)


def operands(B, spread, g):
    """Operator-form inputs of the encoder: one query per token, its reference point the token's
    own centre, offsets = the initial grid (mmcv's init_weights of sampling_offsets) [+ N(0, 8 px)],
    uniform attention weights (zero logits)."""
    th = torch.arange(8, dtype=torch.float32) * (2.0 * math.pi / 8)
    grid = torch.stack([th.cos(), th.sin()], -1)
    grid = (grid / grid.abs().max(-1, keepdim=True)[0]).view(8, 1, 1, 2).repeat(1, 3, 4, 1)
    for i in range(4):
        grid[:, :, i, :] *= i + 1
    off = grid[None, None].repeat(B, SN, 1, 1, 1, 1)                    # [B][N][8][L][4][2], pixels
    if spread:
        off = off + 8.0 * torch.randn(B, SN, 8, 3, 4, 2, generator=g)
    refs = []
    for h, w in SHAPES:
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5,
                                torch.arange(w, dtype=torch.float32) + 0.5, indexing="ij")
        refs.append(torch.stack([xx.reshape(-1) / w, yy.reshape(-1) / h], -1))
    ref = torch.cat(refs, 0)
    norm = torch.tensor([[w, h] for h, w in SHAPES], dtype=torch.float32)
    loc = ref[None, :, None, None, None, :] + off / norm[None, None, None, :, None, :]
    aw = torch.full((B, SN, 8, 3, 4), 1.0 / 12.0)
    ss = torch.tensor(SHAPES, dtype=torch.int64)
    starts = torch.cat([ss.new_zeros(1), (ss[:, 0] * ss[:, 1]).cumsum(0)[:-1]])
    value = torch.randn(B, SN, 256, generator=g)
    gout = torch.randn(B, SN, 256, generator=g)
    return [t.to(DEV).contiguous() for t in (value, ss, starts, loc, aw, gout)]


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters            # ms per call


def summary(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4),
                n=len(xs))


def kernels(reps, iters):
    from pairnet_amd import hip
    g = torch.Generator().manual_seed(0)
    out = []
    for B in (1, 2):
        nbytes = hip.msda_bwd_det_scratch_bytes(B, SN, SN, 3)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        for name, spread in (("init grid", False), ("init + N(0, 8 px)", True)):
            value, ss, starts, loc, aw, gout = operands(B, spread, g)
            gv = torch.zeros_like(value)
            gl, ga = torch.empty_like(loc), torch.empty_like(aw)
            atomic = lambda: hip.msda_bwd(value, 256, ss, starts, loc, aw, gout, gv, gl, ga, B, SN, SN, 3)
            det = lambda: hip.msda_bwd_det(value, 256, ss, starts, loc, aw, gout, gv, gl, ga, B, SN, SN,
                                           3, scratch=scratch)
            for fn in (atomic, det):
                for _ in range(3):
                    fn()
            ta, td = [], []
            for _ in range(reps):
                ta.append(timed(atomic, iters))
                td.append(timed(det, iters))
            # the two entries' grad_value on these operands (from zero): the reordered sum's distance
            gv.zero_(); atomic(); a = gv.clone()
            gv.zero_(); det(); d = gv.clone()
            torch.cuda.synchronize()
            rec = dict(B=B, offsets=name, scratch_bytes=nbytes, atomic_ms=summary(ta), det_ms=summary(td),
                       max_abs_diff=float((a - d).abs().max()), max_abs=float(a.abs().max()))
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def trainer(reps, iters, H=96, W=128):
    """`TailTrainer` scope "all": two trainers on two heads / backbones built alike, deterministic
    off and on, stepped alternately.  96 x 128: the batch of two of tests/test_train_gpu.py; any
    other size: one image with the ground truth of tools/train_step_probe.py (12 objects, 10
    relations, masks at twice the C2 map's size)."""
    import pairnet_amd as P
    g = torch.Generator().manual_seed(2)
    cfg = P.pairnet_head_cfg()
    cfg.pop("type")
    small = (H, W) == (96, 128)
    B = 2 if small else 1
    x = torch.randn(B, 3, H, W, generator=g).to(DEV)
    pts = [torch.rand(1, 12544, 2, generator=g) for _ in range(B)]
    if small:
        metas = [dict(img_shape=(H, W, 3), scale_factor=[2.0] * 4)] * 2
        gt_labels = [torch.tensor([3, 17, 90, 120, 3]), torch.tensor([5, 60, 7])]
        gt_rels = [torch.tensor([[0, 1, 5], [2, 3, 17], [1, 0, 56], [4, 2, 5], [0, 1, 9]]),
                   torch.tensor([[0, 1, 2], [2, 1, 30]])]
        masks = [torch.rand(len(l), H, W, generator=g) > 0.6 for l in gt_labels]
    else:
        G, T = 12, 10
        Hh, Wh = 2 * ((H + 3) // 4), 2 * ((W + 3) // 4)
        metas = [dict(img_shape=(H, W, 3), scale_factor=[2.083] * 4)]
        masks = [(torch.rand(G, Hh // 8, Wh // 8, generator=g) > 0.7).to(DEV)
                 .repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()]
        gt_labels = [torch.randint(0, 133, (G,), generator=g)]
        gt_rels = [torch.stack([torch.randint(0, G, (T,), generator=g),
                                torch.randint(0, G, (T,), generator=g),
                                torch.randint(1, 57, (T,), generator=g)], 1)]
    steps = {}
    for det in (False, True):
        head = P.CrossHead2(**cfg)
        head.init_weights(seed=3)
        head.to(DEV)
        torch.manual_seed(0)
        bb = P.ResNet50Hip().to(DEV)
        tr = P.TailTrainer(head, lr=1e-3, backbone=bb, deterministic=det)
        steps[det] = (lambda tr=tr: tr.step(x, metas, gt_rels, gt_labels, masks, point_coords=pts))
        for _ in range(3):
            steps[det]()
    t = {False: [], True: []}
    for _ in range(reps):
        for det in (False, True):
            t[det].append(timed(steps[det], iters))
    rec = dict(trainer="TailTrainer scope all, %d x %d x %d" % (B, H, W), atomic_step_ms=summary(t[False]),
               det_step_ms=summary(t[True]))
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="alternations (at least 3)")
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--train-hw", default="96,128", help="image size of the trainer's batch of two")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 3:
        sys.exit("--reps: at least three alternations")
    if not torch.cuda.is_available():
        sys.exit("msda_bwd_det_probe measures on an MI355X; there is no CPU path")
    result = {} if args.no_kernels else dict(kernels=kernels(args.reps, args.iters))
    if not args.no_trainer:
        h, w = (int(v) for v in args.train_hw.split(","))
        result["trainer"] = trainer(args.reps, max(args.iters // 4, 3), h, w)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
