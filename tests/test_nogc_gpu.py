"""GPU: the no-graph-constraint ranking (`pn_nogc_triplets_f32`, csrc/nogc.hip) against the numpy
restatement tests/nogc_ref.py -- triplets, rows, count equal, scores bitwise equal -- the box IoU
statistic (`pn_eval_iou_best_boxes`) against `nogc_ref.iou_bbox`, and `TripletEvaluator` /
`StreamingEvaluator` with `nogc` / `iou` against tests/golden/nogc_boxes.npz (recorded from the
reference) and against each other."""
import ctypes

import numpy as np
import pytest
import torch

import nogc_ref as N
from oracle import evaluation as OE
from test_nogc_refs import (EMPTY, KS, golden, golden_dataset, golden_lists, scene, thresholds)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run_rank(scores, labels, rel, t, K=100, ld=5):
    """The kernel's five outputs as numpy arrays (whole, the tail past `count` included)."""
    from pairnet_amd import hip
    R, C1 = rel.shape
    det = np.full((2 * R, ld), 7.0, np.float32)                   # (boxes / padding: not read)
    det[:, 4] = scores
    ar = torch.arange(R, dtype=torch.int32, device=DEV)
    i32 = lambda *s: torch.full(s, 12345, device=DEV, dtype=torch.int32)
    trip, srow, orow, count = i32(K, 3), i32(K), i32(K), i32(1)
    score = torch.full((K,), 9.0, device=DEV, dtype=torch.float32)
    hip.nogc_triplets(_dev(det), ld, _dev(labels), _dev(rel), ar, ar + R, R, C1, t, K, trip,
                      srow, orow, score, count)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (trip, srow, orow, score, count)]


def _check_rank(scores, labels, rel, t, K=100, ld=5):
    R = rel.shape[0]
    pairs = np.stack([np.arange(R), np.arange(R) + R], 1)
    ref = N.nogc_rank(scores, labels, pairs, rel, t, K)
    trip, srow, orow, score, count = _run_rank(scores, labels, rel, t, K, ld)
    n = ref["count"]
    assert int(count[0]) == n == min(K, R * t)
    assert np.array_equal(trip[:n], ref["triplets"])
    assert np.array_equal(srow[:n], ref["sub_rows"]) and np.array_equal(orow[:n], ref["obj_rows"])
    assert np.array_equal(score[:n].view(np.uint32), ref["scores"].view(np.uint32))   # bitwise
    assert (trip[n:] == -1).all() and (srow[n:] == -1).all() and (orow[n:] == -1).all()
    assert (score[n:].view(np.uint32) == 0).all()
    return trip, ref


def _random_case(seed, R, C1, tie_free=True):
    """Random scores; `tie_free`: drawn again until all products differ (at n = 5600 about every
    second draw of float32 products has a pair of equal ones; at n = 65536 every draw has, and
    the tie rule of the restatement decides)."""
    rng = np.random.default_rng(seed)
    while True:
        scores = rng.random(2 * R).astype(np.float32)
        rel = rng.random((R, C1)).astype(np.float32)
        pairs = np.stack([np.arange(R), np.arange(R) + R], 1)
        if not tie_free or N.tie_free(scores, pairs, rel):
            return scores, rng.integers(1, 151, 2 * R), rel


# production shapes (VG C1 = 51, PSG C1 = 57; all predicates, a cut of 3, a cut of 1), n < K
# (count = 9, the tail filled), the smallest call, n = K exactly and n just above K
@pytest.mark.parametrize("R,C1,t", [(100, 51, 50), (100, 57, 56), (100, 57, 3), (100, 57, 1),
                                    (3, 4, 3), (1, 2, 1), (25, 5, 4), (26, 5, 4)])
def test_ranking_equals_the_restatement(R, C1, t):
    scores, labels, rel = _random_case(R * 1000 + C1, R, C1)
    _check_rank(scores, labels, rel, t, K=100)


def test_ranking_larger_shapes_and_a_padded_row_stride():
    """`det` with ld = 5 (above) and padded to ld = 8; a smaller K; the two wider register
    variants of the kernel (n > 8192, n > 24576) up to the largest n the entry accepts."""
    scores, labels, rel = _random_case(5, 100, 57)
    _check_rank(scores, labels, rel, 56, ld=8)
    _check_rank(scores, labels, rel, 3, K=20, ld=8)
    for R, C1, t in ((300, 57, 56), (300, 57, 2), (1024, 65, 64), (1024, 65, 5)):
        s2, l2, r2 = _random_case(R, R, C1, tie_free=False)
        _check_rank(s2, l2, r2, t)


def test_cut_of_one_is_the_graph_constrained_predicate():
    from pairnet_amd import hip
    scores, labels, rel = _random_case(11, 100, 57)
    trip, ref = _check_rank(scores, labels, rel, 1)
    ptrip = torch.empty(100, 3, device=DEV, dtype=torch.int32)
    pscore = torch.empty(100, device=DEV, dtype=torch.float32)
    hip.pred_triplets(_dev(labels), _dev(rel), ptrip, pscore, 100, 57)
    ptrip = ptrip.cpu().numpy()
    assert sorted(ref["row"].tolist()) == list(range(100))        # every pair once
    assert np.array_equal(trip[np.argsort(ref["row"])], ptrip)


def test_tie_rule():
    """Pins THIS LIBRARY's rule, not numpy's (whose default sort leaves ties unspecified): in a
    row and in the ranking the smaller (r, c) wins.  Scores quantised to 1/8, rows of zeros,
    equal pair scores."""
    rng = np.random.default_rng(3)
    for R, C1, t in ((100, 57, 56), (100, 57, 3), (100, 51, 1), (40, 9, 2)):
        scores = (rng.integers(0, 9, 2 * R) / 8).astype(np.float32)
        scores[R:] = scores[:R]                                   # equal pair scores
        scores[:4] = scores[R:R + 4] = 1.0
        rel = (rng.integers(0, 9, (R, C1)) / 8).astype(np.float32)
        rel[1] = 0.0                                              # rows of zeros
        rel[R - 1] = 0.0
        rel[2] = 1.0                                              # a row of equal scores
        _check_rank(scores, rng.integers(1, 151, 2 * R), rel, t)
    zeros = np.zeros((100, 57), np.float32)                       # nothing but ties
    trip, ref = _check_rank(np.ones(200, np.float32), np.arange(200), zeros, 56)
    assert ref["row"].tolist() == [0] * 56 + [1] * 44             # (the restatement's own rule)
    assert ref["pred"].tolist() == list(range(1, 57)) + list(range(1, 45))
    assert trip[:, 1].tolist() == ref["pred"].tolist()


def test_bad_arguments_return_minus_one():
    from pairnet_amd import hip
    lib = hip.lib()
    R, C1, K = 100, 57, 100
    buf = torch.zeros(16384, device=DEV, dtype=torch.int64)       # 128 KB, operands 8 KB apart
    at = lambda kb: ctypes.c_void_p(buf.data_ptr() + 1024 * kb)   # (rel_dists: 23 KB from 16)
    good = [at(0), 5, at(8), at(16), at(48), at(56), R, C1, 56, K, at(64), at(72), at(80), at(88),
            at(96), None]
    assert lib.pn_nogc_triplets_f32(*good) == 0
    for i in (0, 2, 3, 4, 5, 10, 11, 12, 13, 14):                 # NULL operands
        args = list(good)
        args[i] = None
        assert lib.pn_nogc_triplets_f32(*args) == -1, i
    for i, v in ((1, 4), (6, 0), (6, 1171), (7, 1), (8, 0), (8, 57), (9, 0), (9, 101)):
        args = list(good)                                         # ld < 5, R, n = 65576, C1,
        args[i] = v                                               # t outside [1, C1 - 1], K
        assert lib.pn_nogc_triplets_f32(*args) == -1, (i, v)
    good = [at(0), 5, at(8), 100, at(16), 4, at(48), 3, at(56), at(64), None]
    assert lib.pn_eval_iou_best_boxes(*good) == 0
    for i in (0, 2, 4, 6, 8, 9):
        args = list(good)
        args[i] = None
        assert lib.pn_eval_iou_best_boxes(*args) == -1, i
    for i, v in ((1, 3), (3, 0), (5, 3), (7, 0)):
        args = list(good)
        args[i] = v
        assert lib.pn_eval_iou_best_boxes(*args) == -1, (i, v)
    torch.cuda.synchronize()


def _iou_kernel(pred_labels, pbox, ld, gt_labels, gbox):
    from pairnet_amd import hip
    R, nobj = pred_labels.shape[0] // 2, gt_labels.shape[0]
    det = np.zeros((2 * R, ld), np.float32)
    det[:, :4] = pbox
    valid = torch.full((2 * nobj,), 9, device=DEV, dtype=torch.uint8)
    best = torch.full((2 * nobj,), -1.0, device=DEV, dtype=torch.float64)
    hip.eval_iou_best_boxes(_dev(det), ld, _dev(pred_labels.astype(np.int64)), R,
                            _dev(gbox.astype(np.float32)), 4, _dev(gt_labels.astype(np.int32)),
                            nobj, valid, best)
    return valid.cpu().numpy().reshape(2, nobj), best.cpu().numpy().reshape(2, nobj)


def test_iou_kernel_alone():
    rng = np.random.default_rng(4)
    R = 7                                                         # (odd, not the reference's 100)
    gt_labels = np.array([5, 9, 6])
    gbox = np.array([[10, 10, 50, 60], [0, 0, 30, 30], [100, 100, 140, 180]], np.float32)
    pred_labels = rng.integers(20, 30, 2 * R)
    xy = rng.uniform(0, 100, (2 * R, 2))
    pbox = np.concatenate([xy, xy + rng.uniform(5, 60, (2 * R, 2))], 1).astype(np.float32)
    # class 5: on both sides, a zero-area box FIRST (IoU 0), then overlapping ones, the best in
    # the middle; class 9: nowhere (valid 0); class 6: on the subject side only
    for r, b in ((0, [20, 20, 20, 20]), (2, [12, 10, 50, 58]), (5, [30, 30, 80, 90]),
                 (R + 1, [20, 20, 20, 20]), (R + 6, [0, 0, 50, 60])):
        pred_labels[r], pbox[r] = 5, b
    pred_labels[3], pbox[3] = 6, [100, 100, 140, 170]
    for ld in (4, 5, 8):
        valid, best = _iou_kernel(pred_labels, pbox, ld, gt_labels, gbox)
        sub, obj = N.iou_bbox(gt_labels, pred_labels, gbox, pbox)
        assert valid.tolist() == [[1, 0, 1], [1, 0, 0]]
        assert np.array_equal(best[0][valid[0] == 1], np.asarray(sub, np.float64))
        assert np.array_equal(best[1][valid[1] == 1], np.asarray(obj, np.float64))
        assert (best[valid == 0] == 0).all() and 0.9 < best[0, 0] < 1 and best[0, 2] == 0.875
    # n_obj = 1; a class whose only prediction is the degenerate box: valid, IoU exactly 0
    pred_labels[:] = 21
    pred_labels[4], pbox[4] = 5, [20, 20, 20, 20]
    valid, best = _iou_kernel(pred_labels, pbox, 5, gt_labels[:1], gbox[:1])
    sub, obj = N.iou_bbox(gt_labels[:1], pred_labels, gbox[:1], pbox)
    assert valid.tolist() == [[1], [0]] and best.tolist() == [[0.0], [0.0]]
    assert sub == [0.0] and obj == []


def _result(s):
    return (_dev(s["det"]), _dev(s["labels"]), torch.from_numpy(s["rel_pairs"]), None, None,
            _dev(s["rel_dists"]))


@pytest.fixture(scope="module")
def device_evals():
    """`TripletEvaluator.evaluate_boxes(nogc=(3, C1 - 1), iou=True)` of the four fixture scenes
    (shared, never written)."""
    from pairnet_amd.evaluation import TripletEvaluator
    out = []
    for i in range(4):
        s = scene(i)
        out.append(TripletEvaluator().evaluate_boxes(
            _result(s), s["gt_rels"], s["gt_labels"], s["gt_boxes"], nogc=thresholds(i), iou=True))
    return out


@pytest.mark.parametrize("i", range(4))
def test_evaluate_boxes_equals_the_golden(device_evals, i):
    z, s, out = golden(), scene(i), device_evals[i]
    ref = OE.evaluate_boxes(s["labels"], s["rel_pairs"], s["rel_dists"], s["det"][:, :4],
                            s["gt_rels"], s["gt_labels"], s["gt_boxes"])
    for k in ("pred_to_gt", "phrdet_pred_to_gt", "sgdet_recall", "phrdet_recall"):
        assert out[k] == ref[k], k                                # the old part is untouched
    for t in thresholds(i):
        for pre in ("", "phrdet_"):
            key = pre + "nogc@%d" % t
            assert out[key + "_pred_to_gt"] == golden_lists(i, key), key
            assert len(out[key + "_pred_to_gt"]) == 100
            want = {k: float(z["s%d.%s.recall" % (i, key)][j]) for j, k in enumerate(KS)}
            assert out[key + "_recall"] == want, key
    for side in ("sub_iou", "obj_iou"):                           # bitwise: float64 of the float32
        want = z["s%d.%s" % (i, side)]
        assert out[side].dtype == np.float64 and want.dtype == np.float32
        assert np.array_equal(out[side], want.astype(np.float64)), side
        assert np.array_equal(out[side].astype(np.float32).view(np.uint32), want.view(np.uint32))
    from pairnet_amd.evaluation import TripletEvaluator
    empty = TripletEvaluator().evaluate_boxes(_result(s), np.zeros((0, 3), int), s["gt_labels"],
                                              s["gt_boxes"], nogc=True, iou=True)
    C1 = s["rel_dists"].shape[1]
    assert empty["nogc@%d_recall" % (C1 - 1)] is None and "sub_iou" not in empty
    assert len(empty["nogc@%d_pred_to_gt" % (C1 - 1)]) == 100


PARENT_KEYS = {"images", "skipped", "sgdet_recall", "sgdet_mean_recall", "sgdet_mean_recall_list",
               "phrdet_recall", "phrdet_mean_recall", "phrdet_mean_recall_list"}


def _add(ev, idx, i, lo=0, **kw):
    if i is None:                                                 # an image with G = 0
        s = scene(lo)
        ev.add_boxes(_result(s), np.zeros((0, 3), int), s["gt_labels"], s["gt_boxes"], index=idx,
                     **kw)
    else:
        s = scene(i)
        ev.add_boxes(_result(s), s["gt_rels"], s["gt_labels"], s["gt_boxes"], index=idx, **kw)


@pytest.mark.parametrize("lo", [0, 2])
def test_streaming_boxes_equal_the_host_path_and_the_golden(device_evals, lo):
    from pairnet_amd.evaluation import SceneGraphMetrics, StreamingEvaluator
    ts = thresholds(lo)
    C1 = ts[1] + 1
    host = SceneGraphMetrics(C1 - 1, nogc=ts)                     # the host path
    for i in (lo, lo + 1):
        host.add(device_evals[i], scene(i)["gt_rels"])
    host.add(EMPTY, np.zeros((0, 3), int))
    want = host.summary()
    order = [(0, lo), (1, None), (2, lo + 1)]
    ev = StreamingEvaluator(C1 - 1, nogc=ts)
    for idx, i in order:
        _add(ev, idx, i, lo, iou=True)
    got = ev.summary()
    assert got == want                                            # exactly: keys and floats
    assert got["nogc"] == golden_dataset(C1, "both", ts)
    assert got["images"] == 2 and got["skipped"] == 1 and "subject-IoU" in got
    one = StreamingEvaluator(C1 - 1, nogc=True)                   # the reference's default
    for idx, i in order:
        _add(one, idx, i, lo)
    assert one.summary()["nogc"] == golden_dataset(C1, "default", (C1 - 1,))
    assert "subject-IoU" not in one.summary()
    # two ranks
    a, b, c = (StreamingEvaluator(C1 - 1, nogc=ts) for _ in range(3))
    _add(a, 2, lo + 1, lo, iou=True)
    _add(b, 0, lo, lo, iou=True)
    _add(b, 1, None, lo, iou=True)
    c.merge([a.state(), b.state()])
    assert c.summary() == want and np.array_equal(c.state(), ev.state())
    # issued on a side stream, summarised on the default stream
    side = torch.cuda.Stream(device=DEV)
    sv = StreamingEvaluator(C1 - 1, nogc=ts)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for idx, i in order:
            _add(sv, idx, i, lo, iou=True)
    assert sv.summary() == want
    # without nogc and iou: the parent's keys and values (the oracle's lists through the
    # unchanged host aggregation), and the parent's state blob
    plain, old = StreamingEvaluator(C1 - 1), SceneGraphMetrics(C1 - 1)
    for idx, i in order:
        _add(plain, idx, i, lo)
    for i in (lo, lo + 1):
        s = scene(i)
        old.add(OE.evaluate_boxes(s["labels"], s["rel_pairs"], s["rel_dists"], s["det"][:, :4],
                                  s["gt_rels"], s["gt_labels"], s["gt_boxes"]), s["gt_rels"])
    old.add(EMPTY, np.zeros((0, 3), int))
    assert plain.summary() == old.summary() and set(plain.summary()) == PARENT_KEYS
    blob = plain.state()
    assert int(blob[0]) == 0x5345 and blob.shape[0] == 5 + 2 * (4 + 7 * C1) + 1
    assert {k: v for k, v in got.items() if k in PARENT_KEYS} == old.summary()


def test_add_boxes_with_nogc_and_iou_reads_nothing_back(monkeypatch):
    """`add_boxes` enqueues and returns: no tensor is brought to the host (the count of ranked
    triplets is known without reading it), and torch's synchronisation check stays silent."""
    from pairnet_amd.evaluation import StreamingEvaluator, TripletEvaluator
    s = scene(2)
    result = _result(s)
    ev = StreamingEvaluator(56, nogc=(3, 56))
    _add(ev, 0, 2, 2, iou=True)                                   # warm-up
    torch.cuda.synchronize()

    def refuse(name):
        def f(*args, **kw):
            raise AssertionError("host wait: " + name)
        return f
    with monkeypatch.context() as m:
        for name in ("cpu", "item", "numpy", "tolist"):
            m.setattr(torch.Tensor, name, refuse("Tensor." + name))
        with pytest.raises(AssertionError, match="host wait"):    # the check can see a wait
            TripletEvaluator().evaluate_boxes(result, s["gt_rels"], s["gt_labels"], s["gt_boxes"],
                                              nogc=True)
        ev.add_boxes(result, s["gt_rels"], s["gt_labels"], s["gt_boxes"], index=1, iou=True)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.add_boxes(result, s["gt_rels"], s["gt_labels"], s["gt_boxes"], index=2, iou=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    recs = ev.records()
    for i in (1, 2):
        for k in ("hits", "counts", "sub_iou", "obj_iou"):
            assert np.array_equal(recs[i][k], recs[0][k]), (i, k)
        for t in (3, 56):
            assert np.array_equal(recs[i]["nogc_hits"][t], recs[0]["nogc_hits"][t]), (i, t)
