"""What one training iteration of the Swin detector costs on one MI355X (pair-net_amd/train.py with a
SwinTransformerHip backbone): ms per `TailTrainer.step` at 800x1333, one image,

  * `frozen`: the head + pixel decoder's encoder path trained, the Swin backbone frozen (its
    features computed once, resident in HBM) -- the step without a backbone backward;
  * `stage4`: from the image, the backbone's last stage + norm3 trained as
    configs/mask2former/pairnet_swinb.py configures it (frozen_stages=3, SwinBackboneGrad);

and, separately, the stage-4 tape alone (stage_input + taped forward + backward, HIP events).
Prints one JSON line.  Usage: python tools/swin_train_step_probe.py [--swin B|L] [--steps N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pairnet_amd import TailTrainer, build_detector, pairnet_swin  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--swin", default="B", choices=("B", "L"))
ap.add_argument("--steps", type=int, default=10)
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
det = build_detector(pairnet_swin(args.swin))
det.bbox_head.init_weights(seed=0)
det.to(dev)
head, net = det.bbox_head, det.backbone
B, H, W = 1, 800, 1333
g = torch.Generator().manual_seed(3)
img = torch.randn(B, 3, H, W, generator=g).to(dev)
feats = [f.clone(memory_format=torch.preserve_format) for f in net(img)]      # frozen backbone
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


def timed(tr, inp, steps):
    for _ in range(3):
        tr.step(inp, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        vals = tr.step(inp, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps, vals


out = {"what": "TailTrainer.step, Swin-%s detector, 800x1333, one image; ms per step over %d steps "
               "(device wait at both ends); `stage4_tape_ms`: SwinBackboneGrad stage_input + taped "
               "forward + backward of one step (HIP events)" % (args.swin, args.steps)}
for scope in ("frozen", "stage4"):
    tr = TailTrainer(head, train_decoder=True, train_pixel_decoder=True,
                     backbone=net if scope == "stage4" else None)
    ms, vals = timed(tr, img if scope == "stage4" else feats, args.steps)
    out[scope] = {"ms_per_step": ms,
                  "trained_parameters": int(sum(v.numel() for v in tr.params.values())),
                  "loss": {k: float(v) for k, v in vals.items()}}
    if scope == "stage4":
        tape = tr.bb_tape
        out[scope]["backbone_parameters"] = int(sum(
            v.numel() for k, v in tr.params.items() if k.startswith("backbone.")))
        c5 = feats[3].permute(0, 2, 3, 1)
        d = torch.randn(c5.shape, generator=g).to(dev).permute(0, 3, 1, 2)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        with torch.no_grad():
            net(img)
            for i in range(2):                       # (the second one is timed)
                ev[0].record()
                tape.forward(tape.stage_input())
                ev[1].record()
                tape.backward(d)
                ev[2].record()
        torch.cuda.synchronize()
        out[scope]["stage4_tape_ms"] = {"taped_forward": ev[0].elapsed_time(ev[1]),
                                        "backward": ev[1].elapsed_time(ev[2])}
print(json.dumps(out))
