"""Writes tests/golden/baseline_loss.npz: seeded inputs and injected draws of two small cases of the
sibling head's full loss, the 30-key loss dict and the fp32 autograd gradients (with respect to
`rel`, `subject_scores`, `object_scores`) of the reference's OWN `CrossHeadBaseline.loss`
(relation_heads/baseline.py:446-907 with OldIdMatcher, approaches/matcher.py:279-351, and
MultilabelCrossEntropy, losses/seg_losses.py:47-57), the same in float64 from the restatement
(tests/baseline_loss_ref.py) with its magnitudes, the matched pairs, and the reference's measured
error ratio per output, |ref32 - ref64| / (2^-24 mag).  The reference is imported at run time from
its own tree, as oracle/make_golden.py does; only data is written.

    python tools/make_baseline_loss_golden.py

A case is written only if the reference's fp32 and float64 runs agree on every assignment."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import baseline_loss_ref as BR
    import seg_loss_ref as S
    blob = {}
    for name, shape in BR.FIXTURE_CASES.items():
        c = BR.full_case(**shape)
        seg64, r64 = BR.run_whole(c)
        seg32, r32 = BR.run_whole(c, torch.float32, grad=False)
        out32, g32, _ = BR.run_reference(c, torch.float32)
        out64, g64, _ = BR.run_reference(c, torch.float64)
        assert torch.equal(seg64["matched"], seg32["matched"]), name
        for b in range(shape["B"]):
            for i in (0, 1):
                assert np.array_equal(r64["pairs"][b][i], r32["pairs"][b][i]), (name, b)
        for k in BR.NAMES:       # the restatement IS the reference in float64
            assert abs(float(out64[k]) - float(r64["losses"][k])) <= 1e-12, (name, k)
        pre = name + "."
        blob[pre + "shape"] = np.array([shape[k] for k in ("L", "B", "Q", "C", "Cr", "h", "w", "Np")])
        for k in ("cls", "mask", "rel", "sub", "obj"):
            blob[pre + k] = c[k].numpy()
        for b in range(shape["B"]):
            blob[pre + "gt_labels.%d" % b] = c["gt_labels"][b].numpy()
            blob[pre + "gt_masks.%d" % b] = c["gt_masks"][b].numpy()
            blob[pre + "gt_rels.%d" % b] = c["gt_rels"][b].numpy()
            blob[pre + "pairs.%d" % b] = np.stack(r64["pairs"][b]).astype(np.int64)
        for l in range(shape["L"]):
            for b in range(shape["B"]):
                blob[pre + "assign.%d.%d" % (l, b)] = c["points"]["assign"][l][b].numpy()
            blob[pre + "candidates.%d" % l] = c["points"]["candidates"][l].numpy()
            blob[pre + "tail.%d" % l] = c["points"]["tail"][l].numpy()
        blob[pre + "matched"] = seg64["matched"].numpy()
        blob[pre + "pos"], blob[pre + "r_labels"] = r64["pos"].numpy(), r64["r_labels"].numpy()
        names = sorted(out32)
        assert len(names) == 3 * shape["L"] + 3
        blob[pre + "names"] = np.array(names)
        v64 = dict(seg64["losses"], **r64["losses"])
        m64 = dict(seg64["mags"], **r64["mags"])
        l32 = np.array([float(out32[k]) for k in names], np.float32)
        l64 = np.array([float(v64[k]) for k in names])
        mag = np.array([float(m64[k]) for k in names])
        blob[pre + "loss32"], blob[pre + "loss64"], blob[pre + "loss_mag"] = l32, l64, mag
        blob[pre + "loss_ratio"] = np.abs(l32 - l64) / (S.U * np.maximum(mag, S.FLT_MIN))
        for key, a32, a64, amag in (("g_rel", g32[0], r64["g_rel"], r64["g_rel_mag"]),
                                    ("g_sub", g32[1], r64["g_sub"], r64["g_sub_mag"]),
                                    ("g_obj", g32[2], r64["g_obj"], r64["g_obj_mag"])):
            blob[pre + key + "32"] = a32.numpy()
            ratio = (a32.double() - a64).abs() / (S.U * amag + S.FLT_MIN)
            blob[pre + key + "_ratio"] = np.array(float(ratio.max()))
        print(name, {k: round(float(v), 2) for k, v in zip(names, blob[pre + "loss_ratio"]) if k in BR.NAMES},
              {k: float(blob[pre + k + "_ratio"]) for k in ("g_rel", "g_sub", "g_obj")})
    path = BR.GOLDEN
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
