"""CPU: the host side of pairnet_amd.TrainPipeline (config, draws, geometry, boxes / relations)
against the reference's own config file and its own `RelRandomCrop._crop_data`, executed from the
reference tree where it exists (tests/train_pipeline_ref.py) -- integer / float32 work in the
reference's operation order, compared exactly."""
import os

import numpy as np
import pytest

import train_pipeline_ref as R
from oracle import ref_shim

SCALES = [(48, 80), (56, 80)]
CROP = (20, 40)


def _cfg(allow_negative_crop=False):
    from pairnet_amd import train_pipeline_cfg
    cfg = train_pipeline_cfg()
    aug = [t for t in cfg if t["type"] == "AutoAugment"][0]
    aug["policies"][0][0]["img_scale"] = list(SCALES)
    first, crop, second = aug["policies"][1]
    first["img_scale"], second["img_scale"] = [(40, 80), (48, 80)], list(SCALES)
    crop.update(crop_size=CROP, allow_negative_crop=allow_negative_crop)
    return cfg


def _pipe(**kw):
    from pairnet_amd import TrainPipeline
    return TrainPipeline.from_config(_cfg(**kw))


@pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")
def test_restated_train_pipeline_equals_the_reference_config():
    from pairnet_amd import load_config, train_pipeline_cfg
    cfg = load_config(os.path.join(ref_shim.REF_ROOT, "configs/mask2former/pairnet.py"))
    assert cfg.train_pipeline == train_pipeline_cfg()


def test_from_config_reads_the_reference_pipeline_and_refuses_the_rest():
    from pairnet_amd import TrainPipeline, train_pipeline_cfg
    pipe = TrainPipeline.from_config(train_pipeline_cfg())
    assert pipe.flip_ratio == 0.5 and pipe.size_divisor == 1 and pipe.to_rgb
    assert [len(p["scales1"]) for p in pipe.policies] == [11, 3]
    assert pipe.policies[0]["scales1"][0] == (480, 1333) and pipe.policies[0]["crop"] is None
    assert pipe.policies[1]["crop"] == dict(size=(384, 600), allow_negative=False)
    assert pipe.policies[1]["scales2"][-1] == (800, 1333)

    def edited(fn):
        cfg = train_pipeline_cfg()
        fn(cfg, [t for t in cfg if t["type"] == "AutoAugment"][0]["policies"])
        return cfg
    for bad in (lambda c, p: p[0][0].update(keep_ratio=False),
                lambda c, p: p[0][0].update(multiscale_mode="range"),
                lambda c, p: p[1][1].update(crop_type="relative_range"),
                lambda c, p: p[1][1].update(crop_type="absolute"),
                lambda c, p: c[2].update(direction="vertical"),
                lambda c, p: c.insert(3, dict(type="PhotoMetricDistortion")),
                lambda c, p: p[0].append(dict(type="RandomCrop", crop_size=(4, 4)))):
        with pytest.raises(NotImplementedError):
            TrainPipeline.from_config(edited(bad))
    with pytest.raises(RuntimeError):
        TrainPipeline.from_config(train_pipeline_cfg(), device="cpu")


def test_nearest_index_is_opencvs_double_formula():
    from pairnet_amd.train_pipeline import cv_nearest_index
    got = cv_nearest_index(34, 6)
    ifx = 1.0 / (34.0 / 6.0)
    want = [min(int(np.floor(x * ifx)), 5) for x in range(34)]
    assert got.tolist() == want == R.cv_nearest(34, 6).tolist()
    naive = [int(np.floor(x * 6 / 34)) for x in range(34)]
    assert [i for i in range(34) if want[i] != naive[i]] == [17]
    for n_dst, n_src in ((69, 53), (48, 37), (53, 53), (7, 40)):
        assert cv_nearest_index(n_dst, n_src).tolist() == R.cv_nearest(n_dst, n_src).tolist()
        assert cv_nearest_index(n_dst, n_src).max() <= n_src - 1


def test_geometry_on_hand_computed_cases():
    from pairnet_amd import AugParams
    pipe = _pipe()
    # 37 x 53 under (48, 80): factor min(80 / 53, 48 / 37) = 48 / 37 -> 48 x int(68.76 + .5)
    g = pipe.geometry(37, 53, AugParams(False, 0, (48, 80), None, None))
    assert g["size1"] == g["size2"] == g["pad"] == (48, 69) and g["window"] == (0, 0, 48, 69)
    assert g["scale_factor2"] is None and g["scale_factor1"].dtype == np.float32
    assert g["scale_factor1"].tolist() == np.array([69 / 53, 48 / 37] * 2, np.float32).tolist()
    # a 24 x 30 window at (20, 39) of it, then (56, 80): factor min(80 / 30, 56 / 24) = 7 / 3
    g = pipe.geometry(37, 53, AugParams(True, 1, (48, 80), (24, 30, 20, 39), (56, 80)))
    assert g["size1"] == (48, 69) and g["window"] == (20, 39, 24, 30) and g["size2"] == (56, 70)
    assert g["scale_factor2"].tolist() == np.array([70 / 30, 56 / 24] * 2, np.float32).tolist()
    # a crop larger than the image is capped, an offset that would leave it is clipped
    g = pipe.geometry(37, 53, AugParams(False, 1, (48, 80), (60, 100, 5, 7), (48, 80)))
    assert g["window"] == (0, 0, 48, 69) and g["size2"] == (48, 69)
    g = pipe.geometry(37, 53, AugParams(False, 1, (48, 80), (40, 100, 30, 0), (48, 80)))
    assert g["window"] == (8, 0, 40, 69)
    # portrait, and Pad(size_divisor)
    from pairnet_amd import TrainPipeline
    p32 = TrainPipeline(pipe.policies, size_divisor=32)
    g = p32.geometry(53, 37, AugParams(False, 0, (48, 80), None, None))
    assert g["size2"] == (69, 48) and g["pad"] == (96, 64)


def test_sample_params_draws_are_legal_and_repeatable():
    from pairnet_amd.preprocess import rescale_size
    pipe = _pipe()
    seen = set()
    for seed in range(1000):
        H, W = (37, 53) if seed % 2 else (30, 19)      # (30 x 19: the crop range is capped)
        p = pipe.sample_params(H, W, np.random.RandomState(seed))
        assert p == pipe.sample_params(H, W, np.random.RandomState(seed))
        seen.add((p.flip, p.policy))
        assert isinstance(p.flip, bool) and p.policy in (0, 1)
        assert p.scale1 in pipe.policies[p.policy]["scales1"]
        if p.policy == 0:
            assert p.crop is None and p.scale2 is None
            continue
        H1, W1 = rescale_size(H, W, p.scale1)
        ch, cw, oy, ox = p.crop
        assert min(H1, CROP[0]) <= ch <= min(H1, CROP[1]) and min(W1, CROP[0]) <= cw <= min(W1, CROP[1])
        assert 0 <= oy <= H1 - ch and 0 <= ox <= W1 - cw
        assert p.scale2 in SCALES
        assert pipe.geometry(H, W, p)["window"] == (oy, ox, ch, cw)
    assert seen == {(False, 0), (False, 1), (True, 0), (True, 1)}
    never = type(pipe)(pipe.policies, flip_ratio=0.0)
    assert not any(never.sample_params(37, 53, np.random.RandomState(s)).flip for s in range(50))


# (flip, crop (ch, cw, oy, ox) of the 48 x 69 first resize, what it keeps)
CROPS = [(False, (24, 30, 0, 0), "some"), (True, (24, 30, 24, 39), "some"),
         (False, (28, 40, 20, 0), "some"), (False, (48, 69, 0, 0), "all"),
         (False, (20, 20, 0, 16), "none")]


def _targets_equal(got, b, labels, rels, keep):
    assert got["bboxes"].dtype == b.dtype == np.float32 and np.array_equal(got["bboxes"], b)
    assert got["labels"].dtype == labels.dtype and np.array_equal(got["labels"], labels)
    assert got["rels"].dtype == rels.dtype and np.array_equal(got["rels"], rels)
    assert np.array_equal(got["keep"], keep)


@pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")
@pytest.mark.parametrize("flip,crop,keeps", CROPS)
def test_host_crop_logic_equals_the_references_own_crop_data(flip, crop, keeps):
    """pairnet_amd.TrainPipeline.targets and the staged restatement against
    `RelRandomCrop._crop_data` run from the reference's file (boxes, labels, re-indexed
    relations, kept indices), up to the crop: the flip and the first Resize in front of it are
    applied to all three alike."""
    from pairnet_amd import AugParams
    img, pan, ann = R.synthetic_sample(9, hand_placed=True)
    G = len(ann["masks"])
    assert G == 6 and len(ann["rels"]) == 6
    pipe = _pipe()
    # scale2 = the window's own size: the second Resize is the identity, so `targets` ends where
    # `_crop_data` does
    ch, cw, oy, ox = crop
    params = AugParams(flip, 1, (48, 80), crop, (max(ch, cw), min(ch, cw)))
    geo = pipe.geometry(37, 53, params)
    assert geo["size1"] == (48, 69) and geo["size2"] == (ch, cw)
    assert np.array_equal(geo["scale_factor2"], np.ones(4, np.float32))
    got = pipe.targets(ann, params, geo)
    b = R.flip_boxes(ann["bboxes"], 53) if flip else ann["bboxes"].copy()
    b = R.resize_boxes(b, geo["scale_factor1"], (48, 69))
    # (mask g holds g + 1 everywhere: what the reference selected is readable after its crop)
    masks = np.tile(np.arange(1, G + 1, dtype=np.uint8)[:, None, None], (1, 48, 69))
    ref = R.reference_crop_data(np.zeros((48, 69, 3), np.uint8), b, ann["labels"], ann["rels"],
                                masks, (ch, cw), (oy, ox))
    mine = R.crop_targets(b, ann["labels"], ann["rels"], (oy, ox, ch, cw))
    if keeps == "none":
        assert ref is None and got is None and mine is None
        return
    assert ref is not None and got is not None and mine is not None
    kept = ref["gt_bboxes"].shape[0]
    assert (kept == G) if keeps == "all" else (0 < kept < G)
    assert len(ref["gt_rels"]) >= 1 and ref["img_shape"] == (ch, cw, 3)
    assert ref["gt_masks"].masks.shape == (kept, ch, cw)
    ref_keep = ref["gt_masks"].masks[:, 0, 0].astype(np.int64) - 1
    _targets_equal(got, ref["gt_bboxes"], ref["gt_labels"], ref["gt_rels"], ref_keep)
    _targets_equal(dict(bboxes=mine[0], labels=mine[1], rels=mine[2], keep=mine[3]),
                   ref["gt_bboxes"], ref["gt_labels"], ref["gt_rels"], ref_keep)


def test_targets_through_both_resizes_equal_the_staged_pipeline():
    """The whole box path (flip, Resize, crop, Resize; policy 1 too) == the staged restatement,
    which the test above pins to the reference at the crop."""
    from pairnet_amd import AugParams
    img, pan, ann = R.synthetic_sample(9, hand_placed=True)
    pipe = _pipe()
    cases = [AugParams(f, 1, (48, 80), c, (56, 80)) for f, c, _ in CROPS]
    cases += [AugParams(False, 0, (56, 80), None, None), AugParams(True, 0, (48, 80), None, None),
              AugParams(True, 1, (40, 80), (60, 100, 0, 0), (48, 80))]
    some = 0
    for p in cases:
        got = pipe.targets(ann, p, pipe.geometry(37, 53, p))
        want = R.staged_sample(img, pan, ann, p)
        assert (got is None) == (want is None)
        if got is None:
            continue
        some += 1
        _targets_equal(got, want["bboxes"], want["labels"], want["rels"], want["keep"])
    assert some == len(cases) - 1
    # allow_negative_crop keeps the sample with an empty relation list
    loose = _pipe(allow_negative_crop=True)
    p = cases[4]
    got = loose.targets(ann, p, loose.geometry(37, 53, p))
    assert got is not None and got["rels"].shape == (0, 3) and len(got["keep"]) >= 1


def test_public_names_and_abi_entries():
    import re
    import pairnet_amd
    from pairnet_amd import hip
    for name in ("TrainPipeline", "AugParams", "HalfSizeMasks", "train_pipeline_cfg"):
        assert hasattr(pairnet_amd, name) and name in pairnet_amd.api.__all__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    for name in ("pn_augment_image_u8_f32", "pn_augment_resize_crop_u8", "pn_augment_masks_u8"):
        assert name in declared and name in hip.EXPORTS


def test_bad_arguments_are_refused_on_the_host(built_lib):
    """Every refusal of the three entries returns before anything touches a device (this
    machine may have none)."""
    from pairnet_amd import hip
    R.check_bad_arguments(hip.lib())
