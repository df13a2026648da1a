"""Writes tests/golden/seg_loss.npz: seeded inputs and injected draws of two small Mask2Former loss
cases, the loss dict and the fp32 autograd gradients of the reference's OWN `MaskFormerHead.loss`
(panoptic_heads/mask2former_head.py:157-324, maskformer_head.py:181-240,305-354, point_sample.py),
the same in float64 from the restatement (tests/seg_loss_ref.py) and the reference's measured error
ratio per output, |ref32 - ref64| / (2^-24 mag).  The reference is imported at run time from its own
tree, as oracle/make_golden.py does; only data is written.

    python tools/make_seg_loss_golden.py

The reference is run by tests/seg_loss_ref.py's `run_reference()` (what tests/test_seg_loss_refs.py
executes as well), which also holds the [3P] restatements the reference calls."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = dict(a=dict(L=2, B=2, Q=8, C=5, h=13, w=21, Np=50, G=(3, 0), seed=11),
             b=dict(L=2, B=2, Q=8, C=5, h=13, w=21, Np=50, G=(1, 2), seed=12))


from seg_loss_ref import (DiceLoss, SigmoidCE, injected_rand, load_reference,  # noqa: E402,F401
                          run_reference)


def main():
    import seg_loss_ref as S
    blob = {}
    for name, shape in CASES.items():
        c = S.loss_case(**shape)
        r64 = S.whole_loss(c["cls"], c["mask"], c["gt_labels"], c["gt_masks"], c["points"],
                           c["num_classes"], c["class_weight"], c["num_points"])
        out32, gc32, gm32 = run_reference(c, torch.float32)
        rows = r64["mask_rows"]
        h, w = c["mask"].shape[-2:]
        gm32 = gm32.reshape(-1, h, w)
        other = torch.ones(gm32.shape[0], dtype=torch.bool)
        other[rows] = False
        assert float(gm32[other].abs().max() if other.any() else 0.0) == 0.0
        pre = name + "."
        blob[pre + "shape"] = np.array([shape[k] for k in ("L", "B", "Q", "C", "h", "w", "Np")])
        blob[pre + "cls"], blob[pre + "mask"] = c["cls"].numpy(), c["mask"].numpy()
        for b in range(shape["B"]):
            blob[pre + "gt_labels.%d" % b] = c["gt_labels"][b].numpy()
            blob[pre + "gt_masks.%d" % b] = c["gt_masks"][b].numpy()
        for l in range(shape["L"]):
            for b in range(shape["B"]):
                blob[pre + "assign.%d.%d" % (l, b)] = c["points"]["assign"][l][b].numpy()
            blob[pre + "candidates.%d" % l] = c["points"]["candidates"][l].numpy()
            blob[pre + "tail.%d" % l] = c["points"]["tail"][l].numpy()
        blob[pre + "matched"] = r64["matched"].numpy()
        names = sorted(out32)
        blob[pre + "names"] = np.array(names)
        l32 = np.array([float(out32[k]) for k in names], np.float32)
        l64 = np.array([float(r64["losses"][k]) for k in names])
        mag = np.array([float(r64["mags"][k]) for k in names])
        blob[pre + "loss32"], blob[pre + "loss64"], blob[pre + "loss_mag"] = l32, l64, mag
        blob[pre + "loss_ratio"] = np.abs(l32 - l64) / (S.U * np.maximum(mag, S.FLT_MIN))
        # (the float64 gradients are recomputed by the tests from the restatement; the mask
        # gradient's scale carries the tap weights' coordinate error beside the issue's mag)
        for key, g32, g64, gmag in (("g_cls", gc32, r64["g_cls"], r64["g_cls_mag"]),
                                    ("g_mask", gm32[rows], r64["g_mask"],
                                     r64["g_mask_mag"] + S.COORD * r64["g_mask_coord"])):
            blob[pre + key + "32"] = g32.numpy()
            ratio = (g32.double() - g64).abs() / (S.U * gmag + S.FLT_MIN)
            blob[pre + key + "_ratio"] = np.array(float(ratio.max()) if ratio.numel() else 0.0)
        print(name, dict(zip(names, blob[pre + "loss_ratio"].round(2))),
              "g_cls", blob[pre + "g_cls_ratio"], "g_mask", blob[pre + "g_mask_ratio"])
    path = os.path.join(ROOT, "tests", "golden", "seg_loss.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
