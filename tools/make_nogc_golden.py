"""Writes tests/golden/nogc_boxes.npz: the inputs of four box scenes and what the reference's OWN
`SGRecall.calculate_recall`, `SGMeanRecall` and `SGObjectIOU.calculate_iou`
(pairnet/evaluation/sgg_metrics.py:173-343, :669-916, :942-1035) give for them with
`detection_method="bbox"`: the "nogc@t_pred_to_gt" / "phrdet_nogc@t_pred_to_gt" lists, the
per-image recalls, the dataset-level `nogc_result_dict` numbers and the two IoU lists.  The
reference is imported at run time from its own tree (as tests/test_evaluation.py does, with
mmdet's absent `bbox_overlaps` supplied by oracle.evaluation.bbox_overlaps); only data is written.

    python tools/make_nogc_golden.py

Scenes (R = 100): 0, 1 with C1 = 51 (150 object classes), 2, 3 with C1 = 57 (133 classes); scene 3
has one ground-truth relation.  Every scene is recorded for the thresholds (3, C1 - 1); the
dataset-level numbers are recorded per C1 (one evaluator has one predicate count: scenes 0 + 1,
scenes 2 + 3) for the reference's default `(C1 - 1,)` and for `(3, C1 - 1)`.

Conditions, checked here and asserted again by tests/test_nogc_refs.py: all R (C1 - 1) products
of an image pairwise distinct (no ties, so numpy's order is determined); at least 10 nogc matches
per scene; at least one ground-truth relation hit under nogc that the graph-constrained list
misses."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KS = (20, 50, 100)
R = 100
SCENES = (dict(C1=51, classes=150, nobj=8, G=10), dict(C1=51, classes=150, nobj=9, G=7),
          dict(C1=57, classes=133, nobj=8, G=10), dict(C1=57, classes=133, nobj=3, G=1))
OUT = os.path.join(ROOT, "tests", "golden", "nogc_boxes.npz")


def load_reference():
    """The reference's sgg_metrics module, run from where it lies."""
    from oracle import evaluation as OE
    from oracle import ref_shim
    sys.dont_write_bytecode = True
    for name, attrs in (("mmdet", {}), ("mmdet.core", dict(bbox_overlaps=OE.bbox_overlaps)),
                        ("terminaltables", dict(AsciiTable=None))):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
    pkg = types.ModuleType("refevaln")
    pkg.__path__ = [os.path.join(ref_shim.REF_ROOT, "pairnet/evaluation")]
    sys.modules["refevaln"] = pkg
    mods = {}
    for n in ("sgg_eval_util", "sgg_metrics"):
        spec = importlib.util.spec_from_file_location(
            "refevaln." + n, os.path.join(ref_shim.REF_ROOT, "pairnet/evaluation", n + ".py"))
        mods[n] = importlib.util.module_from_spec(spec)
        sys.modules["refevaln." + n] = mods[n]
        spec.loader.exec_module(mods[n])
    return mods["sgg_metrics"]


def box_scene(seed, C1, classes, nobj, G, W=640.0, H=480.0):
    """Ground-truth boxes and predictions derived from them.  Per ground-truth relation j a few
    planted rows: "hit" (the boxes, the predicate on top), "near" (the boxes; a WRONG predicate
    on top, the true one second: the graph-constrained triplet misses, the nogc candidate hits),
    "thr" (subject and object shrunk to IoU 0.5), "low" (IoU 0.45: no match).  Relation 0 gets no
    "hit" / "thr" row: only the nogc ranking finds it."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, [W - 120, H - 120], (nobj, 2))
    wh = rng.uniform(20, 120, (nobj, 2))
    gt_boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    gt_labels = rng.integers(1, classes + 1, nobj)
    pairs = [(s, o) for s in range(nobj) for o in range(nobj) if s != o]
    sel = rng.choice(len(pairs), G, replace=False)
    gt_rels = np.array([[pairs[j][0], pairs[j][1], rng.integers(1, C1)] for j in sel])
    labels = rng.integers(1, classes + 1, 2 * R)
    xy = rng.uniform(0, [W - 60, H - 60], (2 * R, 2))
    boxes = np.concatenate([xy, xy + rng.uniform(5, 60, (2 * R, 2))], 1).astype(np.float32)
    boxes[R - 1] = [10, 10, 10, 10]                               # a degenerate box (zero area)
    rel_dists = rng.random((R, C1)).astype(np.float32)
    rel_dists[:, 0] = 0
    scores = rng.uniform(0.05, 0.6, 2 * R).astype(np.float32)
    if G == 1:
        plan = {0: ["near"] * 12 + ["low"] * 2}
    else:
        plan = {j: ["hit", "near", "thr", "low"] for j in range(G)}
        plan[0] = ["near", "near", "low", "low"]
    r = 0
    for j, (s, o, pr) in enumerate(gt_rels):
        for kind in plan[j]:
            labels[r], labels[R + r] = gt_labels[s], gt_labels[o]
            wrong = 1 + (pr % (C1 - 1))                           # another predicate in [1, C1)
            if kind == "near":
                rel_dists[r, wrong], rel_dists[r, pr] = 2.0, 1.5
            else:
                rel_dists[r, pr] = 2.0
            f = dict(hit=1.0, near=1.0, thr=0.5, low=0.45)[kind]
            for src, dst in ((s, r), (o, R + r)):
                b = gt_boxes[src].copy()
                b[2] = b[0] + (b[2] - b[0]) * f
                boxes[dst] = b
            scores[r], scores[R + r] = rng.uniform(0.9, 1.0, 2)   # planted rows rank high
            r += 1
    det = np.concatenate([boxes, scores[:, None]], 1).astype(np.float32)
    rel_pairs = np.stack([np.arange(R), np.arange(R) + R], 1)
    return dict(labels=labels, rel_pairs=rel_pairs, rel_dists=rel_dists, det=det,
                gt_rels=gt_rels, gt_labels=gt_labels, gt_boxes=gt_boxes)


def make_scenes():
    import nogc_ref as N
    scenes = []
    for i, cfg in enumerate(SCENES):
        seed = 100 * (i + 1)
        while True:                                               # (a tie-free draw)
            sc = box_scene(seed, **cfg)
            if N.tie_free(sc["det"][:, 4], sc["rel_pairs"], sc["rel_dists"]):
                break
            seed += 1
        scenes.append(sc)
    return scenes


def run_reference(M, scenes, thresholds):
    """The reference over `scenes` (one dataset: one C1) with `nogc_thres_num = thresholds`:
    (per image dicts, dataset dict {t: {...}})."""
    thresholds = list(thresholds)
    num_rel = scenes[0]["rel_dists"].shape[1]
    rec = M.SGRecall({}, {}, thresholds, detection_method="bbox")
    rec.register_container("sgdet")
    mr = M.SGMeanRecall({}, {}, thresholds, num_rel, ["bg"] + ["p%d" % i for i in range(1, num_rel)],
                        detection_method="bbox")
    mr.register_container("sgdet")
    glob = dict(iou_thrs=0.5)
    images = []
    for sc in scenes:
        iou = M.SGObjectIOU({}, {}, thresholds, detection_method="bbox")
        iou.register_container("sgdet")
        local = dict(pred_rel_inds=sc["rel_pairs"], rel_scores=sc["rel_dists"],
                     gt_rels=sc["gt_rels"], gt_classes=sc["gt_labels"], gt_boxes=sc["gt_boxes"],
                     pred_classes=sc["labels"], pred_boxes=sc["det"][:, :4],
                     obj_scores=sc["det"][:, 4], pred_masks=None, gt_masks=None)
        rec.calculate_recall(glob, local, "sgdet")
        mr.collect_mean_recall_items(glob, local, "sgdet")
        iou.calculate_iou(glob, local, "sgdet")
        img = dict(pred_to_gt=local["pred_to_gt"], phrdet_pred_to_gt=local["phrdet_pred_to_gt"],
                   sub_iou=np.asarray(iou.result_dict["subject-IoU"], np.float32),
                   obj_iou=np.asarray(iou.result_dict["object-IoU"], np.float32))
        for t in thresholds:
            for mode, pre in (("sgdet", ""), ("phrdet", "phrdet_")):
                img[pre + "nogc@%d_pred_to_gt" % t] = local[pre + "nogc@%d_pred_to_gt" % t]
                img[pre + "nogc@%d_recall" % t] = {
                    k: rec.nogc_result_dict[mode + "_recall"][t][k][-1] for k in KS}
        images.append(img)
    mr.calculate_mean_recall("sgdet")
    data = {}
    for t in thresholds:
        data[t] = {}
        for mode in ("sgdet", "phrdet"):
            data[t][mode + "_recall"] = {
                k: float(np.mean(rec.nogc_result_dict[mode + "_recall"][t][k])) for k in KS}
            data[t][mode + "_mean_recall"] = {
                k: float(mr.nogc_result_dict[mode + "_mean_recall"][t][k]) for k in KS}
            data[t][mode + "_mean_recall_list"] = {
                k: [float(v) for v in mr.nogc_result_dict[mode + "_mean_recall_list"][t][k]]
                for k in KS}
    return images, data


def pack_lists(lists):
    """A list of lists as (pairs [n][2] int32 = (prediction, ground truth), length)."""
    pairs = [(p, g) for p, lst in enumerate(lists) for g in lst]
    return np.asarray(pairs, np.int32).reshape(-1, 2), np.int32(len(lists))


def check_conditions(sc, img, thresholds):
    import nogc_ref as N
    assert N.tie_free(sc["det"][:, 4], sc["rel_pairs"], sc["rel_dists"])
    gc = set(g for lst in img["pred_to_gt"] for g in lst)
    for t in thresholds:
        lists = img["nogc@%d_pred_to_gt" % t]
        assert sum(len(x) for x in lists) >= 10, (t, sum(len(x) for x in lists))
        assert set(g for lst in lists for g in lst) - gc, t


def main():
    M = load_reference()
    scenes = make_scenes()
    blob = dict(ks=np.asarray(KS, np.int32), scenes=np.int32(len(scenes)))
    for lo in (0, 2):                                             # one dataset per C1
        group = scenes[lo:lo + 2]
        C1 = group[0]["rel_dists"].shape[1]
        for cfg, ts in (("default", (C1 - 1,)), ("both", (3, C1 - 1))):
            images, data = run_reference(M, group, ts)
            for t in ts:
                for key, val in data[t].items():
                    arr = np.asarray([val[k] for k in KS], np.float64)
                    blob["ds%d.%s.%d.%s" % (C1, cfg, t, key)] = arr
        for i, (sc, img) in enumerate(zip(group, images), lo):    # (`images` of (3, C1 - 1))
            check_conditions(sc, img, (3, C1 - 1))
            pre = "s%d." % i
            for k, v in sc.items():
                blob[pre + k] = v
            blob[pre + "sub_iou"], blob[pre + "obj_iou"] = img["sub_iou"], img["obj_iou"]
            for t in (3, C1 - 1):
                for p in ("", "phrdet_"):
                    blob[pre + p + "nogc@%d.pairs" % t], blob[pre + p + "nogc@%d.len" % t] = \
                        pack_lists(img[p + "nogc@%d_pred_to_gt" % t])
                    blob[pre + p + "nogc@%d.recall" % t] = np.asarray(
                        [img[p + "nogc@%d_recall" % t][k] for k in KS], np.float64)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **blob)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
