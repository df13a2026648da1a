"""The reference's train pipeline (configs/mask2former/pairnet.py:234-306) STAGED on the CPU, one
stage per function, every intermediate materialised -- what pairnet_amd.TrainPipeline's fused
kernels are compared with, bit for bit.  TEST INFRASTRUCTURE (a helper, not collected).

Composed from parts that are pinned elsewhere: `oracle.preprocess.resize_linear_u8` (OpenCV's
fixed-point INTER_LINEAR), numpy flips and slices, OpenCV's INTER_NEAREST index in its double
formula, `F.pad` + `F.interpolate(mode="nearest")` for frameworks/psgtr.py:126-141, and
`oracle.dataset.load_masks_and_semantic_seg` for the masks at PNG size.  The box / relation side
is restated here stage by stage (mmdet 2.25.1's RandomFlip.bbox_flip, Resize._resize_bboxes,
`RelRandomCrop._crop_data`); `reference_crop_data` runs the reference's OWN rel_randomcrop.py in
place where that tree exists, which is what tests/test_train_pipeline.py pins both this
restatement and the product's host code to.
"""
import functools
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dataset as OD
from oracle import preprocess as OP
from oracle import ref_shim


# ---- pixel stages ---------------------------------------------------------------------------------
def cv_nearest(n_dst, n_src):
    """Source index of each destination index under cv2.resize(INTER_NEAREST)."""
    ifx = 1.0 / (np.float64(n_dst) / np.float64(n_src))
    return np.array([min(int(np.floor(np.float64(x) * ifx)), n_src - 1) for x in range(n_dst)],
                    dtype=np.int64)


def flip_image(img, on):
    return np.ascontiguousarray(img[:, ::-1]) if on else img


def flip_masks(masks, on):
    return np.ascontiguousarray(masks[:, :, ::-1]) if on else masks


def resize_image(img, size):
    return OP.resize_linear_u8(img, size[0], size[1])


def resize_masks(masks, size):
    iy, ix = cv_nearest(size[0], masks.shape[1]), cv_nearest(size[1], masks.shape[2])
    return np.ascontiguousarray(masks[:, iy][:, :, ix])


def crop_image(img, window):
    oy, ox, ch, cw = window
    return np.ascontiguousarray(img[oy:oy + ch, ox:ox + cw])


def crop_masks(masks, window):
    oy, ox, ch, cw = window
    return np.ascontiguousarray(masks[:, oy:oy + ch, ox:ox + cw])


def normalize_pad(img_u8, mean, std, to_rgb, pad_shape):
    """Normalize -> Pad -> ImageToTensor, in oracle/preprocess.py's operation order."""
    x = img_u8.astype(np.float32)
    if to_rgb:
        x = x[..., ::-1]
    stdinv = (1.0 / np.asarray(std, np.float64)).astype(np.float32)
    x = (x - np.asarray(mean, np.float32)) * stdinv
    out = np.zeros((3,) + tuple(pad_shape), np.float32)
    out[:, :x.shape[0], :x.shape[1]] = x.transpose(2, 0, 1)
    return out


def forward_train_masks(masks, Hb, Wb):
    """frameworks/psgtr.py:126-141 on one image's masks [G, h, w] uint8."""
    m = torch.from_numpy(np.ascontiguousarray(masks))
    _, h, w = m.shape
    return F.interpolate(F.pad(m, (0, Wb - w, 0, Hb - h)).unsqueeze(1), size=(Hb // 2, Wb // 2),
                         mode="nearest").squeeze(1)


# ---- box / relation stages ------------------------------------------------------------------------
def flip_boxes(b, W):
    out = b.copy()
    out[:, 0] = W - b[:, 2]
    out[:, 2] = W - b[:, 0]
    return out


def resize_boxes(b, scale_factor, size):
    b = b * scale_factor
    b[:, 0::2] = np.clip(b[:, 0::2], 0, size[1])
    b[:, 1::2] = np.clip(b[:, 1::2], 0, size[0])
    return b


def crop_targets(b, labels, rels, window, allow_negative_crop=False):
    """rel_randomcrop.py:42-83 -> (boxes, labels, rels, kept indices) or None."""
    oy, ox, ch, cw = window
    b = b - np.array([ox, oy, ox, oy], dtype=np.float32)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, cw)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, ch)
    valid = (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])
    left = []
    for s, o, r in np.asarray(rels).tolist():
        if valid[s] and valid[o]:
            left.append([int(valid[:s].sum()), int(valid[:o].sum()), r])
    if not left and not allow_negative_crop:
        return None
    return b[valid], labels[valid], np.array(left, dtype=np.int64).reshape(-1, 3), np.nonzero(valid)[0]


# ---- one image, one batch -------------------------------------------------------------------------
def staged_sample(img, pan, ann, params, mean=OP.MEAN, std=OP.STD, to_rgb=True, size_divisor=1,
                  allow_negative_crop=False):
    """Every stage of one image under `params` (flip, scale1, crop (ch, cw, oy, ox) or None,
    scale2).  Returns None where the crop keeps no relation, else dict(window_u8 (policy 2's
    cropped first resize, else None), final_u8, img [3, Hp, Wp] float32, masks [Gk, H2, W2]
    uint8, bboxes, labels, rels, keep, meta)."""
    H, W = img.shape[:2]
    masks, _ = OD.load_masks_and_semantic_seg(ann, pan)
    x, m = flip_image(img, params.flip), flip_masks(masks, params.flip)
    b = flip_boxes(ann["bboxes"], W) if params.flip else ann["bboxes"].copy()
    labels, rels, keep = ann["labels"], ann["rels"], np.arange(len(ann["masks"]))
    s1 = OP.rescale_size(H, W, params.scale1)
    sf = np.array([s1[1] / W, s1[0] / H, s1[1] / W, s1[0] / H], dtype=np.float32)
    x, m, b = resize_image(x, s1), resize_masks(m, s1), resize_boxes(b, sf, s1)
    window_u8 = None
    if params.crop is not None:
        ch, cw, oy, ox = params.crop
        x = crop_image(x, (oy, ox, ch, cw))
        ch, cw = x.shape[:2]                               # (a crop larger than the image)
        t = crop_targets(b, labels, rels, (oy, ox, ch, cw), allow_negative_crop)
        if t is None:
            return None
        b, labels, rels, keep = t
        m = crop_masks(m[keep], (oy, ox, ch, cw))
        window_u8 = x
        s2 = OP.rescale_size(ch, cw, params.scale2)
        sf = np.array([s2[1] / cw, s2[0] / ch, s2[1] / cw, s2[0] / ch], dtype=np.float32)
        x, m, b = resize_image(x, s2), resize_masks(m, s2), resize_boxes(b, sf, s2)
    H2, W2 = x.shape[:2]
    pad = (-(-H2 // size_divisor) * size_divisor, -(-W2 // size_divisor) * size_divisor)
    meta = dict(ori_shape=(H, W, 3), img_shape=(H2, W2, 3), pad_shape=pad + (3,), scale_factor=sf,
                flip=bool(params.flip), flip_direction="horizontal" if params.flip else None)
    return dict(window_u8=window_u8, final_u8=x, img=normalize_pad(x, mean, std, to_rgb, pad),
                masks=m, bboxes=b, labels=labels, rels=rels, keep=keep, meta=meta)


def collate(staged):
    """mmcv's collate of the staged samples: images zero-padded to the largest, metas given
    `batch_input_shape`; the masks stay per image, at image size (DataContainer, cpu_only)."""
    Hb, Wb = max(s["img"].shape[1] for s in staged), max(s["img"].shape[2] for s in staged)
    img = np.zeros((len(staged), 3, Hb, Wb), np.float32)
    for i, s in enumerate(staged):
        img[i, :, :s["img"].shape[1], :s["img"].shape[2]] = s["img"]
    return dict(img=torch.from_numpy(img),
                img_metas=[dict(s["meta"], batch_input_shape=(Hb, Wb)) for s in staged],
                gt_bboxes=[torch.from_numpy(s["bboxes"]) for s in staged],
                gt_labels=[torch.from_numpy(s["labels"]) for s in staged],
                gt_rels=[torch.from_numpy(s["rels"]) for s in staged],
                gt_masks=[s["masks"] for s in staged])


def metas_equal(a, b):
    if set(a) != set(b):
        return False
    for k in a:
        if isinstance(a[k], np.ndarray):
            if a[k].dtype != b[k].dtype or not np.array_equal(a[k], b[k]):
                return False
        elif a[k] != b[k] or type(a[k]) is not type(b[k]):
            return False
    return True


# ---- the reference's own RelRandomCrop, executed in place -------------------------------------------
class _Masks:
    """Name-only stand-in of mmdet's BitmapMasks: index and crop."""

    def __init__(self, masks):
        self.masks = masks

    def __getitem__(self, idx):
        return _Masks(self.masks[idx])

    def crop(self, bbox):
        x1, y1, x2, y2 = (int(v) for v in bbox)
        return _Masks(self.masks[:, y1:y2, x1:x2])


def _load_rel_random_crop():
    name = "pairnet.datasets.pipelines.rel_randomcrop"
    if name in sys.modules:
        return sys.modules[name].RelRandomCrop
    sys.dont_write_bytecode = True

    class RandomCrop:
        bbox2label = {"gt_bboxes": "gt_labels", "gt_bboxes_ignore": "gt_labels_ignore"}
        bbox2mask = {"gt_bboxes": "gt_masks", "gt_bboxes_ignore": "gt_masks_ignore"}
        bbox_clip_border = True
        recompute_bbox = False

    ref_shim._ensure("mmdet")
    ref_shim._ensure("mmdet.datasets", PIPELINES=ref_shim._Registry())
    ref_shim._ensure("mmdet.datasets.pipelines", RandomCrop=RandomCrop)
    for pkg in ("pairnet", "pairnet.datasets", "pairnet.datasets.pipelines"):
        ref_shim._ensure(pkg)
    return ref_shim._load(name, "pairnet/datasets/pipelines/rel_randomcrop.py").RelRandomCrop


def reference_crop_data(img, bboxes, labels, rels, masks, crop_size, offsets,
                        allow_negative_crop=False):
    """`RelRandomCrop._crop_data` (the reference's file, unmodified) on one resized image with
    the two offsets it would draw fixed to `offsets` = (oy, ox).  Returns its results dict or
    None."""
    cls = _load_rel_random_crop()
    mod = sys.modules[cls.__module__]
    drawn = iter(offsets)

    def randint(lo, hi):
        v = next(drawn)
        assert lo <= v < hi, "offset outside the range the reference draws from"
        return v

    class _Numpy(types.ModuleType):          # numpy with `random.randint` replaced
        def __getattr__(self, key):
            return getattr(np, key)

    fake = _Numpy("numpy")
    fake.random = types.SimpleNamespace(randint=randint)
    real, mod.np = mod.np, fake
    try:
        results = dict(img=img, img_fields=["img"], bbox_fields=["gt_bboxes"],
                       gt_bboxes=bboxes.copy(), gt_labels=labels.copy(), gt_rels=rels.copy(),
                       gt_masks=_Masks(masks), seg_fields=[])
        return cls()._crop_data(results, crop_size, allow_negative_crop)
    finally:
        mod.np = real


# ---- inputs -----------------------------------------------------------------------------------------
# six hand-placed boxes of a 37 x 53 image (x1, y1, x2, y2): four corners, the centre, the whole
BOXES = np.array([[2, 2, 12, 12], [30, 3, 50, 14], [3, 22, 15, 35], [32, 20, 51, 36],
                  [20, 12, 32, 24], [0, 0, 53, 37]], dtype=np.float32)
RELS = np.array([[0, 1, 3], [1, 3, 1], [2, 4, 5], [4, 0, 2], [3, 2, 6], [4, 3, 4]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _first_entry(seed, H, W):
    from pairnet_amd import dataset as P
    from test_dataset import synthetic_psg
    dataset, images = synthetic_psg(seed, n_images=1, H=H, W=W)     # (its one image: train split)
    d = P.load_psg(dataset, "train")["data"][0]
    state = np.random.get_state()
    np.random.seed(seed)
    ann = P.ann_info(d, "train", all_bboxes=True)
    np.random.set_state(state)
    return ann, images[d["pan_seg_file_name"]]


def synthetic_sample(seed, H=37, W=53, hand_placed=False):
    """(img BGR uint8, panoptic PNG RGB uint8, ann) of the first entry of
    test_dataset.synthetic_psg(seed) -- ids above 2^16, its last segment absent from the PNG --:
    `ann` = the product's ann_info(d, "train", all_bboxes=True); with `hand_placed`, its boxes and
    relations are BOXES / RELS (cut to the entry's segments), scaled to the image size.  Seed 9
    has six segments, seed 3 four, seed 5 five."""
    from test_preprocess import _image
    ann, pan = _first_entry(seed, H, W)
    ann = dict(ann, bboxes=ann["bboxes"].copy(), rels=ann["rels"].copy())
    if hand_placed:
        G = len(ann["masks"])
        ann["bboxes"] = (BOXES[:G] * np.array([W / 53, H / 37, W / 53, H / 37], np.float32))
        ann["rels"] = RELS[(RELS[:, 0] < G) & (RELS[:, 1] < G)].copy()
    return _image(seed, H, W), pan, ann


# ---- the refusals of the three entries --------------------------------------------------------------
def check_bad_arguments(lib, img=4096, out=8192, ids=12288):
    """Each refusal include/pairnet_hip.h lists for the train-pipeline entries returns -1.  The
    pointers are integers (never dereferenced on the host; nothing may be launched)."""
    import ctypes
    f3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)

    def image(**kw):
        a = dict(img=img, H=8, W=8, flip=0, out=out, stride=3 * 16 * 16, slot=0, Hn=12, Wn=12,
                 Hmax=16, Wmax=16, mean=f3, std=f3)
        a.update(kw)
        return lib.pn_augment_image_u8_f32(a["img"], a["H"], a["W"], a["flip"], a["out"],
                                           a["stride"], a["slot"], a["Hn"], a["Wn"], a["Hmax"],
                                           a["Wmax"], a["mean"], a["std"], 1, None)

    def window(**kw):
        a = dict(img=img, H=8, W=8, H1=12, W1=12, oy=2, ox=2, out=out, ch=6, cw=6)
        a.update(kw)
        return lib.pn_augment_resize_crop_u8(a["img"], a["H"], a["W"], 0, a["H1"], a["W1"], a["oy"],
                                             a["ox"], a["out"], a["ch"], a["cw"], None)

    def masks(**kw):
        a = dict(png=img, H0=8, W0=8, ids=ids, G=3, H1=12, W1=12, oy=2, ox=2, ch=6, cw=6, H2=10,
                 W2=10, Hb=12, Wb=12, out=out)
        a.update(kw)
        return lib.pn_augment_masks_u8(a["png"], a["H0"], a["W0"], a["ids"], a["G"], 1, a["H1"],
                                       a["W1"], a["oy"], a["ox"], a["ch"], a["cw"], a["H2"], a["W2"],
                                       a["Hb"], a["Wb"], a["out"], None)

    bad = [image(img=None), image(out=None), image(mean=None), image(std=None),
           image(H=0), image(W=-1), image(Hn=0), image(Wn=0), image(slot=-1),
           image(Hmax=11), image(Wmax=11),                     # batch tensor smaller than the image
           image(stride=3 * 16 * 16 - 1), image(out=out + 2),  # stride below a slot; misaligned
           window(img=None), window(out=None), window(H=0), window(W=0), window(H1=0), window(W1=0),
           window(ch=0), window(cw=-3), window(oy=-1), window(ox=-1),
           window(oy=7), window(ox=7), window(ch=11), window(cw=11),     # window leaves the resize
           masks(png=None), masks(ids=None), masks(out=None), masks(H0=0), masks(W0=0), masks(G=0),
           masks(G=257), masks(H1=0), masks(W1=0), masks(ch=0), masks(cw=0), masks(H2=0), masks(W2=0),
           masks(oy=-1), masks(ox=-2), masks(oy=7), masks(ox=7),
           masks(Hb=9), masks(Wb=9),                                      # Hb < H2, Wb < W2
           masks(png=img + 1), masks(out=out + 2), masks(ids=ids + 2)]   # misaligned bases
    assert bad == [-1] * len(bad), bad
