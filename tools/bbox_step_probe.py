"""What one training iteration of the box head costs on one MI355X (pair-net_amd/bbox_train.py;
DESIGN 7b): ms per `PSGTr.box_train_step` at 800 x 1333, one image, from the image (frozen
ResNet-101 -> ChannelMapper -> trunk up to the query selection -> taped relation tail -> loss ->
backward -> clip -> AdamW), in host mode (scipy on the downloaded cost blocks) and with
`device_targets=True` (no host wait), the phases of one step (HIP events) and the peak device
memory.  The parent refuses this config, so there is no earlier figure to compare with.

    python tools/bbox_step_probe.py [steps] [--out profiles/bbox_step.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pairnet_amd import build_detector, cross_r101_vg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("steps", nargs="?", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
B, H, W, G, T = 1, 800, 1333, 12, 10
g = torch.Generator().manual_seed(3)
img = torch.randn(B, 3, H, W, generator=g).to(dev)
metas = [dict(img_shape=(H, W, 3), batch_input_shape=(H, W), scale_factor=[2.083] * 4)] * B
c, s = torch.rand(G, 2, generator=g) * 0.6 + 0.2, torch.rand(G, 2, generator=g) * 0.3 + 0.05
gt_bboxes = [torch.cat([c - s / 2, c + s / 2], -1) * torch.tensor([W, H, W, H], dtype=torch.float32)
             for _ in range(B)]
out = {"what": "PSGTr.box_train_step (cross_r101_vg: ResNet-101, ChannelMapper, CrossHeadBBox), "
               "%d x %d, one image, %d boxes, %d relations; ms per step over %d steps (device wait "
               "at both ends), the phases of one step (HIP events; `loss` holds the cost kernels and "
               "the two assignments -- scipy on the host in host mode) and peak device memory"
               % (H, W, G, T, args.steps)}
hc = cross_r101_vg().model.bbox_head
gt_labels = [torch.randint(0, hc.num_classes, (G,), generator=g) for _ in range(B)]
gt_rels = [torch.stack([torch.randint(0, G, (T,), generator=g), torch.randint(0, G, (T,), generator=g),
                        torch.randint(1, hc.num_relations + 1, (T,), generator=g)], 1)
           for _ in range(B)]
for mode in ("host", "device_targets"):
    det = build_detector(cross_r101_vg().model).to(dev)
    head = det.bbox_head
    tr = det.box_trainer(device_targets=mode == "device_targets")
    torch.cuda.reset_peak_memory_stats(dev)
    for _ in range(3):
        vals = det.box_train_step(img, metas, gt_rels, gt_bboxes, gt_labels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        vals = det.box_train_step(img, metas, gt_rels, gt_bboxes, gt_labels)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / args.steps
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    with torch.no_grad():
        ev[0].record()
        feats = det.extract_feat(img)
        ev[1].record()
        pl = tr._trunk(feats, metas)
        ev[2].record()
        o = tr.tape.forward(pl.q, pl.cls)
        ev[3].record()
        up = {}
        head.loss(dict(cls=pl.cls, sub=o["sub"], obj=o["obj"], rel=o["rel"],
                       importance=o["importance"]), dict(bbox=pl.box), gt_rels, gt_bboxes,
                  gt_labels, metas, grads=up, device_targets=tr.device_targets)
        ev[4].record()
        tr.tape.backward(g_rel=up["rel"], g_importance=up["importance"])
        ev[5].record()
        tr.apply_gradients(guard=head._loss.assign_status if tr.device_targets else None)
        ev[6].record()
    torch.cuda.synchronize()
    names = ("backbone+neck", "trunk", "tape_forward", "loss", "backward", "clip+adamw+refresh")
    out[mode] = dict(ms_per_step=ms, parameters_trained=int(sum(v.numel() for v in tr.params.values())),
                     phases_ms={n: ev[i].elapsed_time(ev[i + 1]) for i, n in enumerate(names)},
                     peak_memory_mib=torch.cuda.max_memory_allocated(dev) / 2 ** 20,
                     losses={k: float(v) for k, v in vals.items()})
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
