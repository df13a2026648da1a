"""SHA-256 digests of what the four training steps compute (pair-net_amd/train.py,
baseline_train.py, bbox_train.py, psgtr2_train.py), for a bitwise A/B of two checkouts: the steps
are reproducible bit for bit wherever no float atomic sits in the backward pass, so a change that
is meant to leave them alone must leave these digests alone.  Public surface only, so the same
file runs in an older checkout.  One configuration per GPU process, one JSON line each (fixed
seeds, the tests' small fixtures): `names`, `seg_off` / `seg_lr` / `seg_wd`, `flat_p0` (as built);
after three steps `flat_p` / `flat_m` / `flat_v` / `clip` / every returned value; `infer` (the
head's inference outputs on the same input: the derived packs were refreshed); after
`write_back()` the head's (and the backbone's) `state_dict()`.

    python tools/trainer_digest.py [--out FILE] [--only tail,baseline_image] [--deterministic]

`--deterministic` passes `deterministic=True` to the configurations with a pixel-decoder tape
(PD_TAPE below): the deformable-attention backward then runs without float atomics
(pn_msda_bwd_det_f32) and those eight become reproducible too; the other six are built exactly as
without the flag.

Stops at the first configuration that fails or exceeds its time limit."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = ("tail", "tail_decoder", "tail_pixel_decoder", "tail_resnet", "tail_swin_last", "tail_swin_all_drop_path",
           "tail_device_targets", "tail_dropout", "baseline_feats", "baseline_image", "bbox_host",
           "bbox_device_targets", "triplet_feats", "triplet_image")
# the configurations whose backward passes pn_msda_bwd_f32's float atomics (labnotes R27.3)
PD_TAPE = ("tail_pixel_decoder", "tail_resnet", "tail_swin_last", "tail_swin_all_drop_path",
           "baseline_feats", "baseline_image", "triplet_feats", "triplet_image")
DEV = "cuda:0"


def digest(x):
    """Tensor (bytes of its fp32 / integer values), or a list / dict of them, or plain data."""
    import torch
    h = hashlib.sha256()
    if isinstance(x, dict):
        x = [(k, digest(v)) for k, v in x.items()]
    if isinstance(x, torch.Tensor):
        h.update(x.detach().cpu().contiguous().numpy().tobytes())
    else:
        h.update(json.dumps([digest(v) if isinstance(v, torch.Tensor) else v for v in x]).encode())
    return h.hexdigest()[:16]


def seeded_head(cls, cfg, seed, **kw):
    from oracle import seeded
    head = cls(**{k: v for k, v in cfg.items() if k != "type"}, **kw)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in head.state_dict().items())
    head.load_state_dict(seeded.seeded_state_dict(shapes, seed))
    return head.to(DEV)


def pyramid(g, B, H, W, chans=(256, 512, 1024, 2048), strides=(4, 8, 16, 32)):
    import torch
    return [torch.randn(B, c, H // s, W // s, generator=g).to(DEV) for c, s in zip(chans, strides)]


def run(name, deterministic=False):
    import torch
    import pairnet_amd as P
    det_kw = dict(deterministic=True) if deterministic and name in PD_TAPE else {}
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(2)
    gt_labels = [torch.tensor([3, 17, 90, 120, 3]), torch.tensor([5, 60, 7])]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 3, 17], [1, 0, 56], [4, 2, 5], [0, 1, 9]]),
               torch.tensor([[0, 1, 2], [2, 1, 30]])]
    bb = None
    if name.startswith("tail_swin"):                  # the small Swin of tests/swin_full_ref.py
        H, W = 50, 70
        cfg = P.pairnet_swin("B")
        cfg["backbone"].update(embed_dims=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8],
                               window_size=4, drop_path_rate=0.2,
                               frozen_stages=3 if name == "tail_swin_last" else -1)
        cfg["bbox_head"] = dict(P.pairnet_head_cfg(in_channels=[32, 64, 128, 256]), strides=[4, 8, 16, 32])
        cfg["bbox_head"].pop("mapper")
        det = P.build_detector(cfg)
        det.bbox_head.init_weights(seed=4)
        det.to(DEV)
        head, bb = det.bbox_head, det.backbone
        kw = dict(drop_path=True, seed=5, decay_mult={"backbone.": 0.0}) if "drop_path" in name else {}
        tr = det.trainer(train_backbone=True, lr=1e-3, **kw, **det_kw)
        x = torch.randn(2, 3, H, W, generator=g).to(DEV)
        metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4, batch_input_shape=(H, W))] * 2
        masks = [(torch.rand(len(l), H, W, generator=g) > 0.6).numpy() for l in gt_labels]
        step = lambda: det.train_step(x, metas, gt_rels, None, gt_labels, masks)
    elif name.startswith("tail"):
        H, W = 96, 128
        cfg = P.pairnet_head_cfg()
        cfg.pop("type")
        head = P.CrossHead2(**cfg)
        head.init_weights(seed=3)
        head.to(DEV)
        x = pyramid(g, 2, H, W)
        metas = [dict(img_shape=(H, W, 3), scale_factor=[2.0] * 4)] * 2
        masks = [torch.rand(len(l), H, W, generator=g) > 0.6 for l in gt_labels]
        pts = [torch.rand(1, 12544, 2, generator=g) for _ in range(2)]
        kw = {"tail_decoder": dict(train_decoder=True),
              "tail_pixel_decoder": dict(train_pixel_decoder=True),
              "tail_device_targets": dict(device_targets=True),
              "tail_dropout": dict(seed=5, dropout=True)}.get(name, {})
        if name == "tail_resnet":
            bb = kw["backbone"] = P.ResNet50Hip().to(DEV)
            x = torch.randn(2, 3, H, W, generator=g).to(DEV)
        tr = P.TailTrainer(head, lr=1e-3, **kw, **det_kw)
        step = lambda: tr.step(x, metas, gt_rels, gt_labels, masks, point_coords=pts)
    elif name.startswith(("baseline", "triplet")):     # the sibling heads, on the same small batch
        H, W = 64, 96
        cc = lambda w: dict(type="ClassificationCost", weight=w)
        tc = dict(num_points=256, oversample_ratio=3.0, importance_sample_ratio=0.75,
                  mask_assigner=dict(type="MaskHungarianAssigner", cls_cost=cc(2.0),
                                     mask_cost=dict(type="CrossEntropyLossCost", weight=5.0, use_sigmoid=True),
                                     dice_cost=dict(type="DiceCost", weight=5.0, pred_act=True, eps=1.0)),
                  sampler=dict(type="MaskPseudoSampler"),
                  id_assigner=dict(type="OldIdMatcher", sub_id_cost=cc(1.0), obj_id_cost=cc(1.0),
                                   r_cls_cost=cc(1.0)))
        if name.startswith("baseline"):
            head = seeded_head(P.CrossHeadBaseline, P.baseline_head_cfg(), 1234, train_cfg=tc)
            trainer = P.BaselineTrainer
        else:
            head = seeded_head(P.PSGTrHead2, P.psgtr2_head_cfg(), 1234)
            trainer = P.PSGTr2Trainer
        head.exact_mask_order = True
        x = pyramid(g, 2, H, W)
        if name.endswith("_image"):
            bb = P.ResNet50Hip().to(DEV)
            x = torch.randn(2, 3, H, W, generator=g).to(DEV)
        metas = [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)] * 2
        masks = [(torch.rand(len(l), H // 2, W // 2, generator=g) > 0.6).to(torch.uint8) for l in gt_labels]
        tr = trainer(head, backbone=bb, lr=1e-3, seed=3, **det_kw)
        step = lambda: tr.step(x, metas, gt_rels, gt_labels, masks)
    else:
        H, W = 128, 160
        head = seeded_head(P.CrossHeadBBox, P.bbox_head_cfg(), 3)
        x = [torch.randn(2, 256, h, w, generator=g).to(DEV) for h, w in ((16, 20), (8, 10), (4, 5), (2, 3))]
        metas = [dict(batch_input_shape=(H, W), img_shape=(H, W, 3), scale_factor=[1.0] * 4)] * 2
        c, s = torch.rand(5, 2, generator=g) * 0.6 + 0.2, torch.rand(5, 2, generator=g) * 0.3 + 0.05
        box = torch.cat([c - s / 2, c + s / 2], -1) * torch.tensor([W, H, W, H], dtype=torch.float32)
        rels = [torch.tensor([[0, 1, 5], [2, 3, 17], [1, 0, 50], [4, 2, 5]]), torch.tensor([[0, 1, 2], [2, 1, 30]])]
        tr = P.BBoxTrainer(head, lr=1e-3, device_targets=name == "bbox_device_targets")
        step = lambda: tr.step(x, metas, rels, [box, box[:3]], [gt_labels[0], gt_labels[1]])
    out = OrderedDict(config=name, names=digest(list(tr.names)), n_names=len(tr.names))
    if deterministic:
        out["deterministic"] = bool(det_kw)
    for k in ("seg_off", "seg_lr", "seg_wd"):
        out[k] = digest(getattr(tr, k))
    out["flat_p0"] = digest(tr.flat_p)
    for _ in range(3):
        vals = step()
    torch.cuda.synchronize()
    for k in ("flat_p", "flat_m", "flat_v", "clip"):
        out[k] = digest(getattr(tr, k))
    out["returned"] = digest({k: vals[k] for k in sorted(vals)})
    feats = x if bb is None else det.extract_feat(x) if name.startswith("tail_swin") else \
        [f.clone(memory_format=torch.preserve_format) for f in bb(x)]
    a, b = head.forward(feats, metas)
    out["infer"] = digest({k: v for d in (a, b) for k, v in sorted(d.items()) if isinstance(v, torch.Tensor)})
    tr.write_back()
    out["head_state"] = digest(head.state_dict())
    if bb is not None:
        out["backbone_state"] = digest(bb.state_dict())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=None, help="run this one configuration in this process")
    ap.add_argument("--only", default=",".join(CONFIGS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=150, help="seconds per configuration")
    ap.add_argument("--deterministic", action="store_true",
                    help="deterministic=True where there is a pixel-decoder tape")
    args = ap.parse_args()
    if args.config:
        run(args.config, args.deterministic)
        sys.exit(0)
    lines = []
    for name in args.only.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", name]
                               + (["--deterministic"] if args.deterministic else []),
                               capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit("%s: no result within %d s; stopping" % (name, args.limit))
        if r.returncode != 0:
            sys.exit("%s: exit status %d; stopping\n%s" % (name, r.returncode, r.stderr[-3000:]))
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
