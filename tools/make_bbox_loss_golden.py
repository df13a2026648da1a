"""Record tests/golden/bbox_loss.npz: the reference's own `CrossHeadBBox.loss`
(pairnet/models/relation_heads/pairnet_bbox_head.py:362-464), run in place through oracle/ref_shim
under the restated [3P] assigner / sampler of tests/bbox_loss_ref.py, on the two small cases
`bbox_loss_ref.GOLDEN_CASES`.  Per case: the inputs, the reference's fp32 losses and fp32 autograd
logit gradients, the float64 ones, the float64 magnitudes (the same computation on absolute values:
mean |element loss| per term; per gradient tensor its largest entry), both matchers' assignments.

A case is written only if the fp32 and the float64 run agree on every assignment and both
assignments' margins (bbox_loss_ref.margin) exceed 1e-3: a condition on the inputs (the seeds in
GOLDEN_CASES were chosen so).  Needs the reference tree; run from the repository root:
    python tools/make_bbox_loss_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bbox_loss_ref as R   # noqa: E402


def record(name, spec, out):
    case = R.make_case(**spec)
    l32, g32, a32 = R.run_reference(case, torch.float32)
    l64, g64, a64 = R.run_reference(case, torch.float64)
    assert len(a32) == len(a64) and all(torch.equal(x, y) for x, y in zip(a32, a64)), \
        "%s: the fp32 and float64 runs assign differently -- choose another seed" % name
    r64, traces, rg64 = R.loss(case, torch.float64, grads=True)
    for k in l64:
        assert abs(float(l64[k]) - float(r64[k])) <= 1e-12 * max(1.0, abs(float(l64[k]))), k
    for b, tr in enumerate(traces):
        m1, m2 = R.margin(tr["box_cost"].numpy()), R.margin(tr["id_cost"].numpy())
        assert min(m1, m2) > 1e-3, "%s image %d: assignment margins %g / %g" % (name, b, m1, m2)
        print("%s image %d: box margin %.4f  id margin %.4f" % (name, b, m1, m2))
    pre = name + "."
    B = case["cls"].shape[0]
    for k in ("cls", "bbox", "sub", "obj", "rel", "importance"):
        out[pre + k] = case[k].numpy()
    for b in range(B):
        out[pre + "gt_bboxes.%d" % b] = case["gt_bboxes"][b].numpy()
        out[pre + "gt_labels.%d" % b] = case["gt_labels"][b].numpy()
        out[pre + "gt_rels.%d" % b] = case["gt_rels"][b].numpy()
        out[pre + "img_shape.%d" % b] = np.asarray(case["img_metas"][b]["img_shape"], np.int64)
        for k in ("box_rows", "box_cols", "triplet_rows", "triplet_cols", "query_of_gt"):
            out[pre + "%s.%d" % (k, b)] = np.asarray(traces[b][k], np.int64)
    out[pre + "batch_shape"] = np.asarray(case["img_metas"][0]["batch_input_shape"], np.int64)
    out[pre + "B"], out[pre + "num_classes"] = np.int64(B), np.int64(case["num_classes"])
    out[pre + "num_relations"] = np.int64(case["num_relations"])
    mags = R.loss_magnitudes(case, traces)
    for k in l64:
        out[pre + k + ".f32"] = l32[k].numpy()
        out[pre + k + ".f64"] = l64[k].numpy()
        out[pre + k + ".mag"] = np.float64(mags[k])
    for k in g64:
        out[pre + "grad." + k + ".f32"] = g32[k].numpy()
        out[pre + "grad." + k + ".f64"] = g64[k].numpy()
        out[pre + "grad." + k + ".mag"] = np.float64(g64[k].abs().max())


def main():
    out = {}
    for name, spec in R.GOLDEN_CASES.items():
        record(name, spec, out)
    os.makedirs(os.path.dirname(R.GOLDEN), exist_ok=True)
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
