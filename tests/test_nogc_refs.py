"""Box evaluation, the no-graph-constraint recalls and the box IoU statistic (CPU part).

tests/nogc_ref.py restates `SGRecall.calculate_recall` :254-343 and `_compute_iou_bbox`
:1133-1178 of pairnet/evaluation/sgg_metrics.py in numpy; here it is compared with the reference
run live (where its tree is present) and with tests/golden/nogc_boxes.npz (recorded from the
reference by tools/make_nogc_golden.py), and the host side of pairnet_amd.evaluation
(`SceneGraphMetrics(nogc=...)`, `host_record`, `StreamingEvaluator.add_host` / `state` / `merge`)
with both.

The fixture's four scenes have two predicate counts (C1 = 51: scenes 0, 1; C1 = 57: scenes 2, 3)
and one evaluator has one, so the dataset-level numbers are those of the two datasets (0 + 1) and
(2 + 3), each once with the reference's default threshold `(C1 - 1,)` and once with `(3, C1 - 1)`."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import nogc_ref as N
from oracle import evaluation as OE
from oracle import ref_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nogc_boxes.npz")
KS = (20, 50, 100)
INPUTS = ("labels", "rel_pairs", "rel_dists", "det", "gt_rels", "gt_labels", "gt_boxes")
_cache = {}


def golden():
    if "z" not in _cache:
        z = np.load(GOLDEN)
        _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def scene(i):
    z = golden()
    return {k: z["s%d.%s" % (i, k)] for k in INPUTS}


def golden_lists(i, key):
    """"nogc@3" / "phrdet_nogc@50" ... of scene i as the reference's list of lists."""
    z = golden()
    out = [[] for _ in range(int(z["s%d.%s.len" % (i, key)]))]
    for p, g in z["s%d.%s.pairs" % (i, key)]:
        out[int(p)].append(int(g))
    return out


def thresholds(i):
    C1 = scene(i)["rel_dists"].shape[1]
    return (3, C1 - 1)


def host_eval(i, ts=None, iou=True):
    """What `TripletEvaluator.evaluate_boxes(..., nogc=ts, iou=True)` returns, from the
    restatements alone (no device)."""
    key = (i, ts, iou)
    if key not in _cache:
        s = scene(i)
        ts_ = thresholds(i) if ts is None else ts
        out = OE.evaluate_boxes(s["labels"], s["rel_pairs"], s["rel_dists"], s["det"][:, :4],
                                s["gt_rels"], s["gt_labels"], s["gt_boxes"])
        out.update(N.evaluate_boxes_nogc(s["labels"], s["rel_pairs"], s["rel_dists"], s["det"],
                                         s["gt_rels"], s["gt_labels"], s["gt_boxes"], ts_))
        if iou:
            sub, obj = N.iou_bbox(s["gt_labels"], s["labels"], s["gt_boxes"], s["det"])
            out["sub_iou"], out["obj_iou"] = np.asarray(sub, np.float64), np.asarray(obj, np.float64)
        _cache[key] = out
    return _cache[key]


def golden_dataset(C1, cfg, ts):
    z = golden()
    out = {}
    for t in ts:
        out[t] = {}
        for mode in ("sgdet", "phrdet"):
            for what in ("_recall", "_mean_recall"):
                v = z["ds%d.%s.%d.%s%s" % (C1, cfg, t, mode, what)]
                out[t][mode + what] = {k: float(v[j]) for j, k in enumerate(KS)}
            v = z["ds%d.%s.%d.%s_mean_recall_list" % (C1, cfg, t, mode)]
            out[t][mode + "_mean_recall_list"] = {k: [float(x) for x in v[j]]
                                                  for j, k in enumerate(KS)}
    return out


EMPTY = dict(pred_to_gt=[], phrdet_pred_to_gt=[], sgdet_recall=None, phrdet_recall=None)


@pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")
def test_restatement_equals_the_reference_run_live():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_nogc_golden as T
    finally:
        sys.path.pop(0)
    M = T.load_reference()
    for lo in (0, 2):
        group = [scene(lo), scene(lo + 1)]
        ts = thresholds(lo)
        C1 = ts[1] + 1
        images, data = T.run_reference(M, group, ts)
        ours = []
        for j, (s, img) in enumerate(zip(group, images)):
            mine = host_eval(lo + j)
            ours.append(mine)
            for t in ts:
                for pre in ("", "phrdet_"):
                    assert mine[pre + "nogc@%d_pred_to_gt" % t] == img[pre + "nogc@%d_pred_to_gt" % t]
                    assert len(img[pre + "nogc@%d_pred_to_gt" % t]) == 100
                    assert mine[pre + "nogc@%d_recall" % t] == img[pre + "nogc@%d_recall" % t]
            sub, obj = N.iou_bbox(s["gt_labels"], s["labels"], s["gt_boxes"], s["det"])
            assert len(sub) == len(img["sub_iou"]) > 0 and len(obj) == len(img["obj_iou"]) > 0
            assert all(a == b for a, b in zip(sub, img["sub_iou"]))
            assert all(a == b for a, b in zip(obj, img["obj_iou"]))
        assert N.dataset_numbers(ours, [s["gt_rels"] for s in group], C1, ts) == data
        # the reference's default threshold alone gives the same numbers for that threshold
        _, data1 = T.run_reference(M, group, (C1 - 1,))
        assert data1[C1 - 1] == data[C1 - 1]


def test_restatement_equals_the_golden_file_and_the_scenes_keep_their_conditions():
    z = golden()
    assert int(z["scenes"]) == 4 and tuple(z["ks"]) == KS
    assert scene(3)["gt_rels"].shape[0] == 1                      # the image with G = 1
    assert [scene(i)["rel_dists"].shape for i in range(4)] == [(100, 51)] * 2 + [(100, 57)] * 2
    for i in range(4):
        s, mine = scene(i), host_eval(i)
        # no ties: numpy's order, hence the reference's lists, are determined
        assert N.tie_free(s["det"][:, 4], s["rel_pairs"], s["rel_dists"])
        gc = set(g for lst in mine["pred_to_gt"] for g in lst)
        for t in thresholds(i):
            for pre in ("", "phrdet_"):
                key = pre + "nogc@%d" % t
                assert mine[key + "_pred_to_gt"] == golden_lists(i, key), (i, key)
                want = {k: float(z["s%d.%s.recall" % (i, key)][j]) for j, k in enumerate(KS)}
                assert mine[key + "_recall"] == want, (i, key)
            lists = golden_lists(i, "nogc@%d" % t)
            assert sum(len(x) for x in lists) >= 10                # the scene really has matches
            # ... and a relation only the no-graph-constraint ranking finds
            assert set(g for lst in lists for g in lst) - gc
        sub, obj = N.iou_bbox(s["gt_labels"], s["labels"], s["gt_boxes"], s["det"])
        assert np.array_equal(np.asarray(sub, np.float32), z["s%d.sub_iou" % i])
        assert np.array_equal(np.asarray(obj, np.float32), z["s%d.obj_iou" % i])
        assert z["s%d.sub_iou" % i].dtype == np.float32 and len(sub) > 0


@pytest.mark.parametrize("lo", [0, 2])
def test_scene_graph_metrics_equals_the_reference_dataset_numbers(lo):
    from pairnet_amd.evaluation import SceneGraphMetrics
    ts = thresholds(lo)
    C1 = ts[1] + 1
    for cfg, nogc in (("both", ts), ("default", True), ("default", C1 - 1)):
        agg = SceneGraphMetrics(C1 - 1, nogc=nogc)
        for i in (lo, lo + 1):
            agg.add(host_eval(i), scene(i)["gt_rels"])
        agg.add(EMPTY, np.zeros((0, 3), int))                      # an image without relations
        summ = agg.summary()
        want = golden_dataset(C1, cfg, ts if cfg == "both" else (C1 - 1,))
        assert summ["nogc"] == want
        assert summ["images"] == 2 and summ["skipped"] == 1
        assert summ["nogc"][C1 - 1]["sgdet_recall"][100] > summ["sgdet_recall"][100]
        assert "subject-IoU" in summ
    plain = SceneGraphMetrics(C1 - 1)
    with_nogc = SceneGraphMetrics(C1 - 1, nogc=ts)
    for i in (lo, lo + 1):
        plain.add(host_eval(i, iou=False), scene(i)["gt_rels"])
        with_nogc.add(host_eval(i, iou=False), scene(i)["gt_rels"])
    ps, ws = plain.summary(), with_nogc.summary()
    assert "nogc" not in ps and "subject-IoU" not in ps
    assert {k: v for k, v in ws.items() if k != "nogc"} == ps      # the rest is untouched


def _stream(C1, nogc, images, **kw):
    from pairnet_amd.evaluation import StreamingEvaluator
    ev = StreamingEvaluator(C1 - 1, nogc=nogc, **kw)
    for idx, i in images:
        if i is None:
            ev.add_host(idx, EMPTY, np.zeros((0, 3), int))
        else:
            ev.add_host(idx, host_eval(i), scene(i)["gt_rels"])
    return ev


@pytest.mark.parametrize("lo", [0, 2])
def test_streaming_add_host_state_and_merge(lo):
    from pairnet_amd.evaluation import SceneGraphMetrics, StreamingEvaluator, host_record
    ts = thresholds(lo)
    C1 = ts[1] + 1
    agg = SceneGraphMetrics(C1 - 1, nogc=ts)
    for i in (lo, lo + 1):
        agg.add(host_eval(i), scene(i)["gt_rels"])
    agg.add(EMPTY, np.zeros((0, 3), int))
    want = agg.summary()
    whole = _stream(C1, ts, [(0, lo), (1, lo + 1), (2, None)])
    assert whole.summary() == want
    assert whole.summary()["nogc"] == golden_dataset(C1, "both", ts)
    rec = whole.records()[0]
    hits, counts, more = host_record(host_eval(lo), scene(lo)["gt_rels"], C1, KS, nogc=ts)
    assert more.shape == (2, 2, 3, C1)
    assert np.array_equal(rec["hits"], hits) and np.array_equal(rec["counts"], counts)
    for j, t in enumerate(ts):
        assert np.array_equal(rec["nogc_hits"][t], more[j])
    assert (more[1, 0, 2] >= hits[0, 2]).all() and more[1, 0, 2, 0] > hits[0, 2, 0]
    # two ranks
    a = _stream(C1, ts, [(1, lo + 1)])
    b = _stream(C1, ts, [(0, lo), (2, None)])
    c = StreamingEvaluator(C1 - 1, nogc=ts)
    c.merge([a.state(), b.state()])
    assert c.summary() == want
    assert np.array_equal(c.state(), whole.state())
    blob = whole.state()
    assert int(blob[0]) == StreamingEvaluator._MAGIC_NOGC != StreamingEvaluator._MAGIC
    assert [int(v) for v in blob[3:8]] == [3, C1, 2, 3, C1 - 1]     # nk, num_rel, thresholds
    # another configuration is refused, in both directions
    with pytest.raises(ValueError, match="configuration"):
        StreamingEvaluator(C1 - 1, nogc=(2, C1 - 1)).merge([blob])
    with pytest.raises(ValueError, match="configuration"):
        StreamingEvaluator(C1 - 1, nogc=(C1 - 1,)).merge([blob])
    with pytest.raises(ValueError, match="configuration"):
        StreamingEvaluator(C1 - 1).merge([blob])
    plain = _stream(C1, None, [(0, lo), (1, lo + 1), (2, None)])
    with pytest.raises(ValueError, match="configuration"):
        StreamingEvaluator(C1 - 1, nogc=ts).merge([plain.state()])
    with pytest.raises(ValueError, match="twice"):
        StreamingEvaluator(C1 - 1, nogc=ts).merge([blob, a.state()])
    # without nogc: the old magic, today's header and record length, no "nogc" in the summary
    pb = plain.state()
    assert int(pb[0]) == 0x5345 and [int(v) for v in pb[1:5]] == [2, 1, 3, C1]
    n_iou = sum(len(host_eval(i)[k]) for i in (lo, lo + 1) for k in ("sub_iou", "obj_iou"))
    assert pb.shape[0] == 5 + 2 * (4 + 7 * C1) + n_iou + 1
    assert "nogc" not in plain.summary()
    assert plain.summary() == {k: v for k, v in want.items() if k != "nogc"}


def test_refusals_come_before_any_device_use():
    from pairnet_amd.evaluation import (SceneGraphMetrics, StreamingEvaluator, TripletEvaluator,
                                        nogc_thresholds)
    assert nogc_thresholds(None, 56, KS) == () and nogc_thresholds(True, 56, KS) == (56,)
    assert nogc_thresholds(3, 56, KS) == (3,) and nogc_thresholds([3, 56], 56, KS) == (3, 56)
    for cls in (SceneGraphMetrics, StreamingEvaluator):
        with pytest.raises(ValueError, match="100"):
            cls(56, ks=(20, 50, 101), nogc=True)                   # k > 100 with nogc
        cls(56, ks=(20, 50, 101))                                  # ... is fine without
        for bad in (0, 57, (3, 0), (1, 2, 3, 4, 5), (), (3, 3)):
            with pytest.raises(ValueError):
                cls(56, nogc=bad)
        cls(56, nogc=(1, 2, 3, 56))
    s = scene(0)                                                   # host tensors: no device
    result = (torch.from_numpy(s["det"]), torch.from_numpy(s["labels"]),
              torch.from_numpy(s["rel_pairs"]), None, None, torch.from_numpy(s["rel_dists"]))
    for ev, nogc in ((TripletEvaluator(ks=(20, 200)), True), (TripletEvaluator(), 0),
                     (TripletEvaluator(), 51), (TripletEvaluator(), (1, 2, 3, 4, 5))):
        with pytest.raises(ValueError):
            ev.evaluate_boxes(result, s["gt_rels"], s["gt_labels"], s["gt_boxes"], nogc=nogc)
    ev = StreamingEvaluator(56, nogc=True)
    with pytest.raises(NotImplementedError, match="sgg_metrics.py:254"):
        ev.add((None,) * 8, s["gt_rels"], s["gt_labels"], None)    # masks under nogc
    with pytest.raises(ValueError, match="predicates"):            # C1 - 1 = 50 under 56
        ev.add_boxes(result, s["gt_rels"], s["gt_labels"], s["gt_boxes"])
    assert ev.state().shape[0] == 3 + 4                            # nothing was added


def test_boundary_declares_the_two_entries():
    from pairnet_amd import build as B
    from pairnet_amd import hip
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_\w+)\s*\(", header))
    for name in ("pn_nogc_triplets_f32", "pn_eval_iou_best_boxes"):
        assert name in declared and name in hip._SIGS and name in hip.EXPORTS, name
        assert not name.startswith("pn_tri_")
    assert len(hip._SIGS["pn_nogc_triplets_f32"][1]) == 16
    assert len(hip._SIGS["pn_eval_iou_best_boxes"][1]) == 11
    for cite in ("sgg_metrics.py:254-343", "sgg_metrics.py:1025-1028, :1133-1178",
                 "`bbox_overlaps` restated from memory, unpinned"):
        assert cite in header, cite
    assert sorted(n for n in declared if n.startswith("pn_tri_")) == \
        ["pn_tri_match_cost_f32", "pn_tri_pair_splits", "pn_tri_targets"]
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION == 34
    assert "nogc" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "nogc.hip"))
    assert callable(hip.nogc_triplets) and callable(hip.eval_iou_best_boxes)
