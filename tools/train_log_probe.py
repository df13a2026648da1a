"""What the device-side training log (pair-net_amd/runner.py `TrainLog`, csrc/train_log.hip) costs
per step on one MI355X: the tail step of tools/train_step_probe.py (`TailTrainer(head,
device_targets=True)`, 800x1333, one image, frozen ResNet-50 features resident) in windows of
`--window` steps, alternately WITHOUT and WITH `log.add(out)` after every step (the window's second
launch and record copy included), each window bracketed by device events; `--repeats` windows of
each kind, medians.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pairnet_amd import CrossHead2, ResNet50Hip, TailTrainer, TrainLog, pairnet_head_cfg  # noqa: E402

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
ap = argparse.ArgumentParser()
ap.add_argument("--window", type=int, default=50)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
cfg = pairnet_head_cfg()
cfg.pop("type")
head = CrossHead2(**cfg)
head.init_weights(seed=0)
head.to(dev)
net = ResNet50Hip().to(dev)
B, H, W = 1, 800, 1333
g = torch.Generator().manual_seed(3)
img = torch.randn(B, 3, H, W, generator=g).to(dev)
feats = [f.clone(memory_format=torch.preserve_format) for f in net(img)]
metas = [dict(img_shape=(H, W, 3), scale_factor=[2.083] * 4)] * B
G, T = 12, 10
Hh, Wh = 4 * feats[0].shape[2] // 2, 4 * feats[0].shape[3] // 2
gt_masks = [(torch.rand(G, Hh // 8, Wh // 8, generator=g) > 0.7).to(dev)
            .repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous() for _ in range(B)]
gt_labels = [torch.randint(0, head.num_classes, (G,), generator=g) for _ in range(B)]
gt_rels = [torch.stack([torch.randint(0, G, (T,), generator=g), torch.randint(0, G, (T,), generator=g),
                        torch.randint(1, head.num_relations + 1, (T,), generator=g)], 1)
           for _ in range(B)]
pts = [torch.rand(1, 12544, 2, generator=g) for _ in range(B)]
tr = TailTrainer(head, device_targets=True)
log = TrainLog(dev, interval=args.window)


def window(with_log):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(args.window):
        out = tr.step(feats, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
        if with_log:
            log.add(out, epoch=1, iter=i + 1, lr=tr.lr)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.window


for kind in (False, True):                        # warm-up of both kinds
    window(kind)
plain, logged = [], []
for _ in range(args.repeats):                     # alternating
    plain.append(window(False))
    logged.append(window(True))
log.flush()
# the two launches alone, back to back on an idle device
out = tr.step(feats, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
torch.cuda.synchronize()
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
for i in range(10 * args.window):
    log.add(out, epoch=1, iter=i + 1, lr=tr.lr)
b.record()
torch.cuda.synchronize()
log.flush()
med = statistics.median
print(json.dumps({
    "what": "TailTrainer(device_targets=True).step, 800x1333, one image, resident features: ms per "
            "step over windows of %d steps (device events), without and with TrainLog.add after "
            "every step, %d alternating windows each" % (args.window, args.repeats),
    "ms_per_step_plain": plain, "ms_per_step_logged": logged,
    "median_plain": med(plain), "median_logged": med(logged),
    "median_difference_us": 1e3 * (med(logged) - med(plain)),
    "log_launches_alone_us_per_step": 1e3 * a.elapsed_time(b) / (10 * args.window),
    "windows_logged": len(log.records)}))
