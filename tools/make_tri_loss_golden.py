"""Writes tests/golden/tri_loss.npz: seeded inputs and injected draws of two small PSGTrHead2 loss
cases, the loss dict and the fp32 autograd gradients of the reference's OWN `PSGTrHead2.loss`
(relation_heads/psgtr_head2.py:447-1018 with `MaskHTriMatcher`, approaches/matcher.py:10-102, and
panoptic_heads/point_sample.py), the same in float64 from the restatement (tests/tri_loss_ref.py)
and the reference's measured error ratio per output, |ref32 - ref64| / (2^-24 mag).  The reference
is imported at run time from its own tree, as tools/make_seg_loss_golden.py does; only data is
written.

    python tools/make_tri_loss_golden.py

The reference is run by tests/tri_loss_ref.py's `run_reference()` (what tests/test_tri_loss_refs.py
executes as well)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import seg_loss_ref as S
    import tri_loss_ref as T
    blob = {}
    for name, shape in T.GOLDEN_CASES.items():
        c = T.tri_case(**shape)
        r64 = T.whole_loss(c)
        out32, g32, pairs = T.run_reference(c, torch.float32)
        B, Q = c["sub"].shape[1:3]
        h, w = c["sub_seg"].shape[-2:]
        rows = r64["mask_rows"]
        assert [p for b in range(B) for p in pairs[b]] == \
            list(zip(r64["matched"][:, 1].tolist(), r64["rel_idx"].tolist()))
        pre = name + "."
        blob[pre + "shape"] = np.array([B, Q, c["num_classes"], c["num_relations"], h, w,
                                        c["num_points"]])
        for k in T._TENSORS:
            blob[pre + k] = c[k].numpy()
        for b in range(B):
            blob[pre + "gt_labels.%d" % b] = c["gt_labels"][b].numpy()
            blob[pre + "gt_masks.%d" % b] = c["gt_masks"][b].numpy()
            blob[pre + "gt_rels.%d" % b] = c["gt_rels"][b].numpy()
            blob[pre + "assign.%d" % b] = c["points"]["assign"][b].numpy()
        for k in T._POINTS:
            blob[pre + k] = c["points"][k].numpy()
        blob[pre + "matched"] = r64["matched"].numpy()
        blob[pre + "rel_idx"] = r64["rel_idx"].numpy()
        blob[pre + "names"] = np.array(T.NAMES)
        l32 = np.array([float(out32[k]) for k in T.NAMES], np.float32)
        l64 = np.array([float(r64["losses"][k]) for k in T.NAMES])
        mag = np.array([float(r64["mags"][k]) for k in T.NAMES])
        blob[pre + "loss32"], blob[pre + "loss64"], blob[pre + "loss_mag"] = l32, l64, mag
        blob[pre + "loss_ratio"] = np.abs(l32 - l64) / (S.U * np.maximum(mag, S.FLT_MIN))
        triples = [("g_" + k, g32[k], r64["g_" + k], r64["g_%s_mag" % k]) for k in ("sub", "obj", "rel")]
        for s, k in enumerate(("sub", "obj")):
            gm = g32[k + "_seg"].reshape(-1, h, w)
            other = torch.ones(gm.shape[0], dtype=torch.bool)
            other[rows] = False
            assert float(gm[other].abs().max()) == 0.0
            sd = r64["sides"][s]
            triples.append(("g_%s_mask" % k, gm[rows], sd["g_mask"],
                            sd["g_mask_mag"] + S.COORD * sd["g_mask_coord"]))
        for key, a32, a64, gmag in triples:
            blob[pre + key + "32"] = a32.numpy()
            ratio = (a32.double() - a64).abs() / (S.U * gmag + S.FLT_MIN)
            blob[pre + key + "_ratio"] = np.array(float(ratio.max()))
        print(name, dict(zip(T.NAMES, blob[pre + "loss_ratio"].round(2))),
              {k: float(blob[pre + k + "_ratio"]) for k, _, _, _ in triples})
    path = T.GOLDEN
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
