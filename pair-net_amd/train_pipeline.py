"""Train-time input pipeline on the MI355X: from a decoded image, its panoptic PNG and
`dataset.ann_info(d, "train", all_bboxes=True)` to the batch dict `PSGTr.train_step` takes.

The reference feeds `PSGTr.forward_train` from mmdet's CPU pipeline
(configs/mask2former/pairnet.py:234-306):

    RandomFlip(0.5) -> AutoAugment[ policy 1: Resize(11 scales)
                                  | policy 2: Resize(3 scales) -> RelRandomCrop -> Resize(11 scales) ]
    -> Normalize -> Pad(size_divisor=1) -> RelsFormatBundle -> Collect -> collate(samples_per_gpu=2)

and `forward_train` then pads every image's masks to the batch tensor and resizes them to half
size (frameworks/psgtr.py:126-141).  Here the random draws (`sample_params`), the sizes
(`geometry`) and the <= 256 boxes / relations (`targets`, numpy like `dataset.ann_info`) are host
code; the per-pixel work is csrc/augment.hip: one launch per image for policy 1 (two for policy
2, whose first Resize is evaluated on the crop window only) and ONE launch per image for all of
its masks, from the PNG straight to the half-size, batch-padded masks the loss consumes -- every
mask stage is a gather, so they compose into one index map per axis and no mask at an
intermediate size is ever written.  No CPU path.

Decoding the JPEG / PNG is the caller's I/O, as in dataset.py.  `gt_semantic_seg` is not
produced (the reference's Collect drops it).
"""
from collections import namedtuple

import numpy as np
import torch

from . import hip
from .preprocess import MEAN, STD, rescale_size

AugParams = namedtuple("AugParams", "flip policy scale1 crop scale2")
AugParams.__doc__ = """One image's draws: flip (bool), policy (index into the AutoAugment
policies), scale1 (the first Resize's img_scale), crop ((ch, cw, oy, ox) as drawn, or None for
a policy without a crop), scale2 (the second Resize's img_scale, or None)."""


class HalfSizeMasks:
    """Ground-truth masks that are ALREADY what `PSGTr.forward_train`'s preparation yields for
    the batch tensor of size `batch_shape` = (Hb, Wb): `masks` uint8 [G, Hb // 2, Wb // 2] on the
    device.  `PSGTr._prepare_gt_masks` passes such an entry through after checking its shape."""

    def __init__(self, masks, batch_shape):
        self.masks, self.batch_shape = masks, (int(batch_shape[0]), int(batch_shape[1]))


def cv_nearest_index(n_dst, n_src):
    """OpenCV INTER_NEAREST's source index of every destination index (what mmcv.imresize(...,
    interpolation="nearest") = BitmapMasks.rescale / resize samples): in doubles,
    min(floor(x * (1.0 / (n_dst / n_src))), n_src - 1) -- not floor(x * n_src / n_dst).  The
    host-side statement of csrc/pixel_maps.h `cv_nearest`."""
    ifx = 1.0 / (float(n_dst) / float(n_src))
    x = np.arange(n_dst, dtype=np.float64)
    return np.minimum(np.floor(x * ifx).astype(np.int64), n_src - 1)


def _scales(t):
    s = t["img_scale"]
    s = [tuple(v) for v in s] if isinstance(s[0], (list, tuple)) else [tuple(s)]
    if not t.get("keep_ratio", True):
        raise NotImplementedError("Resize(keep_ratio=True) only")
    if len(s) > 1 and t.get("multiscale_mode", "range") != "value":
        raise NotImplementedError("Resize(multiscale_mode='value') only")
    if t.get("ratio_range") is not None:
        raise NotImplementedError("Resize(ratio_range=...)")
    return s


def _policy(transforms):
    kinds = [t["type"] for t in transforms]
    if kinds == ["Resize"]:
        return dict(scales1=_scales(transforms[0]), crop=None, scales2=None)
    if kinds == ["Resize", "RelRandomCrop", "Resize"]:
        c = transforms[1]
        if c.get("crop_type", "absolute") != "absolute_range":
            raise NotImplementedError("RelRandomCrop(crop_type='absolute_range') only")
        lo, hi = (int(v) for v in c["crop_size"])
        if not 0 < lo <= hi:
            raise ValueError("crop_size: (min, max) with 0 < min <= max")
        if not transforms[2].get("override", False):
            raise NotImplementedError("the Resize after the crop must set override=True")
        return dict(scales1=_scales(transforms[0]),
                    crop=dict(size=(lo, hi), allow_negative=bool(c.get("allow_negative_crop", False))),
                    scales2=_scales(transforms[2]))
    raise NotImplementedError("AutoAugment policy %s: [Resize] or [Resize, RelRandomCrop, Resize]"
                              % kinds)


class TrainPipeline:
    def __init__(self, policies, flip_ratio=0.5, mean=MEAN, std=STD, to_rgb=True, size_divisor=1,
                 device="cuda:0"):
        self.policies = [dict(p) for p in policies]
        self.flip_ratio, self.to_rgb, self.size_divisor = float(flip_ratio), bool(to_rgb), size_divisor
        if not 0.0 <= self.flip_ratio <= 1.0 or not self.policies:
            raise ValueError("flip_ratio in [0, 1] and at least one policy")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TrainPipeline runs on an MI355X only; there is no CPU path")
        self._mean = (torch.tensor(mean, dtype=torch.float32),
                      (1.0 / torch.tensor(std, dtype=torch.float64)).to(torch.float32))
        self._slots = {}               # one grow-only byte buffer per slot
        self.rejected = []             # samples of the last batch() whose crop kept no relation

    @classmethod
    def from_config(cls, train_pipeline, device="cuda:0"):
        """Build from the reference's `train_pipeline` list (config.train_pipeline_cfg())."""
        kw, policies = dict(device=device), None
        for t in train_pipeline:
            kind = t["type"]
            if kind == "RandomFlip":
                if t.get("direction", "horizontal") != "horizontal":
                    raise NotImplementedError("RandomFlip(direction='horizontal') only")
                r = t.get("flip_ratio")
                if isinstance(r, (list, tuple)):
                    raise NotImplementedError("RandomFlip with one flip_ratio only")
                kw["flip_ratio"] = 0.0 if r is None else r
            elif kind == "AutoAugment":
                policies = [_policy(p) for p in t["policies"]]
            elif kind == "Normalize":
                kw.update(mean=t["mean"], std=t["std"], to_rgb=t.get("to_rgb", True))
            elif kind == "Pad":
                if t.get("size") is not None or t.get("pad_to_square", False):
                    raise NotImplementedError("Pad(size_divisor=...) only")
                kw["size_divisor"] = t.get("size_divisor") or 1
            elif kind in ("LoadImageFromFile", "LoadPanopticSceneGraphAnnotations",
                          "RelsFormatBundle", "Collect"):
                continue               # caller I/O, and the formats `batch` returns
            else:
                raise NotImplementedError("train pipeline step %s" % kind)
        if policies is None:
            raise NotImplementedError("a train pipeline without AutoAugment policies")
        kw.setdefault("flip_ratio", 0.0)
        return cls(policies, **kw)

    # ---- host side ----------------------------------------------------------------------------
    def sample_params(self, H, W, rng):
        """One image's draws from `rng` (a numpy.random.RandomState).  Order and distributions
        follow mmdet 2.25.1: RandomFlip's direction choice; AutoAugment's policy choice; Resize's
        scale index; RandomCrop._get_crop_size's crop h, then crop w (absolute_range:
        randint(min(dim, lo), min(dim, hi) + 1)); `_crop_data`'s offset h, then offset w
        (rel_randomcrop.py:29-32); the second Resize's scale index.  UNPINNED: mmdet is not
        available to check against, the order is restated from its published source; the RNG
        stream itself is not claimed to reproduce mmdet's."""
        flip = bool(rng.choice(2, p=[self.flip_ratio, 1.0 - self.flip_ratio]) == 0)
        policy = int(rng.randint(0, len(self.policies)))
        p = self.policies[policy]
        scale1 = p["scales1"][int(rng.randint(len(p["scales1"])))]
        if p["crop"] is None:
            return AugParams(flip, policy, scale1, None, None)
        H1, W1 = rescale_size(H, W, scale1)
        lo, hi = p["crop"]["size"]
        ch = int(rng.randint(min(H1, lo), min(H1, hi) + 1))
        cw = int(rng.randint(min(W1, lo), min(W1, hi) + 1))
        oy = int(rng.randint(0, max(H1 - ch, 0) + 1))
        ox = int(rng.randint(0, max(W1 - cw, 0) + 1))
        scale2 = p["scales2"][int(rng.randint(len(p["scales2"])))]
        return AugParams(flip, policy, scale1, (ch, cw, oy, ox), scale2)

    def geometry(self, H, W, params):
        """Every intermediate size of an H x W image under `params`: dict(ori (H, W), size1 (the
        first Resize), window (oy, ox, ch, cw) inside it -- the crop size capped at the resized
        image, the offset clipped so that the window stays inside --, size2 (the last Resize;
        = size1 without a crop), pad (after Pad), scale_factor1 / scale_factor2 (float32 [4],
        mmdet's w, h, w, h; scale_factor2 None without a crop))."""
        H1, W1 = rescale_size(H, W, params.scale1)
        sf1 = np.array([W1 / W, H1 / H, W1 / W, H1 / H], dtype=np.float32)
        if params.crop is None:
            window, (H2, W2), sf2 = (0, 0, H1, W1), (H1, W1), None
        else:
            ch, cw, oy, ox = (int(v) for v in params.crop)
            if ch <= 0 or cw <= 0:
                raise ValueError("crop size must be positive")
            ch, cw = min(ch, H1), min(cw, W1)
            oy, ox = min(max(oy, 0), H1 - ch), min(max(ox, 0), W1 - cw)
            window = (oy, ox, ch, cw)
            H2, W2 = rescale_size(ch, cw, params.scale2)
            sf2 = np.array([W2 / cw, H2 / ch, W2 / cw, H2 / ch], dtype=np.float32)
        d = self.size_divisor
        return dict(ori=(H, W), size1=(H1, W1), window=window, size2=(H2, W2),
                    pad=(-(-H2 // d) * d, -(-W2 // d) * d), scale_factor1=sf1, scale_factor2=sf2)

    def targets(self, ann, params, geo):
        """The boxes, labels and relations of one image through the pipeline (numpy, <= 256 rows):
        mmdet's RandomFlip.bbox_flip, Resize._resize_bboxes (times the float32 scale_factor, clip
        to img_shape), `RelRandomCrop._crop_data` (rel_randomcrop.py:42-83: offset, clip,
        valid_inds, relations with both ends valid re-indexed by the count of valid boxes before
        them, labels / masks selected by valid_inds), Resize again.  Returns dict(bboxes, labels,
        rels, keep) -- `keep`: indices into ann["masks"] of the segments whose masks remain -- or
        None when the crop keeps no relation and allow_negative_crop is False."""
        b = np.array(ann["bboxes"], dtype=np.float32)
        labels, rels = ann["labels"], ann["rels"]
        keep = np.arange(len(ann["masks"]))
        (H0, W0), (H1, W1), (H2, W2) = geo["ori"], geo["size1"], geo["size2"]
        if params.flip:
            f = b.copy()
            f[..., 0::4] = W0 - b[..., 2::4]
            f[..., 2::4] = W0 - b[..., 0::4]
            b = f
        b = b * geo["scale_factor1"]
        b[:, 0::2] = np.clip(b[:, 0::2], 0, W1)
        b[:, 1::2] = np.clip(b[:, 1::2], 0, H1)
        if params.crop is not None:
            oy, ox, ch, cw = geo["window"]
            b = b - np.array([ox, oy, ox, oy], dtype=np.float32)
            b[:, 0::2] = np.clip(b[:, 0::2], 0, cw)
            b[:, 1::2] = np.clip(b[:, 1::2], 0, ch)
            valid = (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])
            before = np.concatenate([[0], np.cumsum(valid)])     # valid boxes before index i
            left = [[before[r[0]], before[r[1]], r[2]] for r in rels
                    if valid[r[0]] and valid[r[1]]]
            if not left and not self.policies[params.policy]["crop"]["allow_negative"]:
                return None
            rels = np.array(left, dtype=np.int64).reshape(-1, 3)
            b, labels, keep = b[valid, :], labels[valid], valid.nonzero()[0]
            b = b * geo["scale_factor2"]
            b[:, 0::2] = np.clip(b[:, 0::2], 0, W2)
            b[:, 1::2] = np.clip(b[:, 1::2], 0, H2)
        return dict(bboxes=b, labels=labels, rels=rels, keep=keep)

    # ---- device side --------------------------------------------------------------------------
    def _u8(self, a, what):
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a))
        if a.dtype != torch.uint8 or a.dim() != 3 or a.shape[2] != 3:
            raise RuntimeError("%s must be uint8 (H, W, 3)" % what)
        return a.to(self.device, non_blocking=True).contiguous()

    @torch.no_grad()
    @hip.on_device
    def batch(self, samples, slot=0, params=None, rng=None):
        """`samples`: k tuples (img uint8 (H, W, 3) BGR, panoptic PNG uint8 (H, W, 3) RGB,
        ann = dataset.ann_info(d, "train", all_bboxes=True)) -> the collated dict
        `PSGTr.train_step(data_batch, None)` takes: img float32 (k, 3, Hb, Wb) zero-padded to the
        largest image, img_metas, gt_bboxes / gt_labels / gt_rels (host tensors, mmdet's dtypes)
        and gt_masks (`HalfSizeMasks`, device).  `params`: one AugParams per sample, else drawn
        from `rng`.  Everything lives in ONE grow-only buffer per `slot` (views of it: the next
        batch of the same slot overwrites them) and is written on the current stream, so a
        caller can queue the next batch on a side stream under the running step; no allocation
        once the largest batch has passed (for inputs that are device tensors already).

        Returns None -- nothing launched, `self.rejected` lists the sample indices -- when a
        sample's crop keeps no relation (allow_negative_crop=False): mmdet's dataset then draws
        another image, and so does the caller."""
        if params is None:
            if rng is None:
                raise ValueError("batch() needs `params` or an `rng` to draw them from")
            params = [self.sample_params(int(s[0].shape[0]), int(s[0].shape[1]), rng)
                      for s in samples]
        if len(params) != len(samples) or not samples:
            raise ValueError("one AugParams per sample")
        geo, tgt = [], []
        for (img, pan, ann), p in zip(samples, params):
            H, W = int(img.shape[0]), int(img.shape[1])
            if tuple(pan.shape[:2]) != (H, W):
                raise ValueError("image %s and panoptic PNG %s differ in size"
                                 % ((H, W), tuple(pan.shape[:2])))
            if len(ann["masks"]) != len(ann["bboxes"]):
                raise ValueError("ann: one box per segment (ann_info(..., all_bboxes=True))")
            g = self.geometry(H, W, p)
            geo.append(g)
            tgt.append(self.targets(ann, p, g))
        self.rejected = [i for i, t in enumerate(tgt) if t is None]
        if self.rejected:
            return None
        k = len(samples)
        Hb, Wb = max(g["pad"][0] for g in geo), max(g["pad"][1] for g in geo)
        Ho, Wo = Hb // 2, Wb // 2
        # layout of the slot's buffer (bytes, every part 256-aligned): batch tensor | segment
        # ids | per image: its masks, its policy-2 window
        up = lambda n: -(-n // 256) * 256
        ids = [[int(ann["masks"][j]["id"]) for j in t["keep"]] for (_, _, ann), t in zip(samples, tgt)]
        if max(len(v) for v in ids) > 256:
            raise ValueError("at most 256 segments per image")
        off_ids = up(k * 3 * Hb * Wb * 4)
        cur = off_ids + up(4 * sum(len(v) for v in ids))
        off_mask, off_win = [], []
        for v, g in zip(ids, geo):
            off_mask.append(cur)
            cur += up(len(v) * Ho * Wo)
            off_win.append(cur)
            if g["scale_factor2"] is not None:
                cur += up(g["window"][2] * g["window"][3] * 3)
        buf = self._slots.get(slot)
        if buf is None or buf.numel() < cur:
            # (allocated on the current stream: the caching allocator hands the old block back
            # to this stream's pool, where every earlier use of it was queued)
            buf = self._slots[slot] = torch.empty(cur, device=self.device, dtype=torch.uint8)
        out = buf[:k * 3 * Hb * Wb * 4].view(torch.float32).view(k, 3, Hb, Wb)
        n_ids = sum(len(v) for v in ids)
        dev_ids = buf[off_ids:off_ids + 4 * n_ids].view(torch.int32)
        if n_ids:
            dev_ids.copy_(torch.tensor([i for v in ids for i in v], dtype=torch.int32),
                          non_blocking=True)
        metas, masks, first = [], [], 0
        for i, ((img, pan, _), p, g) in enumerate(zip(samples, params, geo)):
            img, pan = self._u8(img, "img"), self._u8(pan, "the panoptic PNG")
            (H, W), (H1, W1), (H2, W2) = g["ori"], g["size1"], g["size2"]
            oy, ox, ch, cw = g["window"]
            if g["scale_factor2"] is None:
                hip.augment_image(img, H, W, p.flip, out, i, H2, W2, self._mean[0], self._mean[1],
                                  self.to_rgb)
            else:
                win = buf[off_win[i]:off_win[i] + ch * cw * 3].view(ch, cw, 3)
                hip.augment_resize_crop(img, H, W, p.flip, H1, W1, oy, ox, win)
                hip.augment_image(win, ch, cw, False, out, i, H2, W2, self._mean[0],
                                  self._mean[1], self.to_rgb)
            G = len(ids[i])
            m = buf[off_mask[i]:off_mask[i] + G * Ho * Wo].view(G, Ho, Wo)
            if G:
                hip.augment_masks(pan, dev_ids[first:first + G], p.flip, (H1, W1), g["window"],
                                  (H2, W2), (Hb, Wb), m)
            first += G
            masks.append(HalfSizeMasks(m, (Hb, Wb)))
            sf = g["scale_factor1"] if g["scale_factor2"] is None else g["scale_factor2"]
            metas.append(dict(ori_shape=(H, W, 3), img_shape=(H2, W2, 3),
                              pad_shape=g["pad"] + (3,), scale_factor=sf, flip=bool(p.flip),
                              flip_direction="horizontal" if p.flip else None,
                              batch_input_shape=(Hb, Wb)))
        return dict(img=out, img_metas=metas,
                    gt_bboxes=[torch.from_numpy(np.ascontiguousarray(t["bboxes"])) for t in tgt],
                    gt_labels=[torch.from_numpy(np.ascontiguousarray(t["labels"])) for t in tgt],
                    gt_rels=[torch.from_numpy(np.ascontiguousarray(t["rels"])) for t in tgt],
                    gt_masks=masks)

    def __call__(self, img_bgr_u8, pan_rgb_u8, ann, params=None, rng=None, slot=0):
        """One image: `batch` of one sample (None when its crop keeps no relation)."""
        return self.batch([(img_bgr_u8, pan_rgb_u8, ann)], slot=slot,
                          params=None if params is None else [params], rng=rng)
