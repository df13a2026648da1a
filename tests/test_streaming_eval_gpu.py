"""GPU: `StreamingEvaluator` on the MI355X -- the records csrc/evaluate.hip leaves on the device
equal the numpy restatement (`evaluation.host_record`) of the oracle's match lists exactly, the
IoU statistic equals `oracle.evaluation.iou_panseg` value for value (NaN included), `add()`
never waits for the device, records added on several streams arrive whole, and
`dist.multi_gpu_test` returns the host path's metrics."""
import numpy as np
import pytest
import torch

from oracle import evaluation as OE
from test_evaluation import _box_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUM_REL = 57
# R = 10 lies below every k, R = 200 has k = 100 < R, G = 70 is more than one wavefront of
# relations, G = 1 / n_obj = 2 the smallest image that is not skipped
SHAPES = [(100, 9, 7), (100, 1, 2), (10, 9, 7), (200, 70, 9)]


def _crafted(seed, R, G, nobj, H=61, W=83):
    """A `_scene`-style image (tests/test_evaluation.py) at a size whose last mask word is
    partial (61 * 83 = 5063 = 79 * 64 + 7), for any R / G: rectangles as ground truth,
    predictions planted on rows spread over [0, R) -- exact hits, wrong predicates, IoU near
    0.5 -- and, from G = 9 on: relation 1 duplicates relation 0 (one prediction hits both),
    predicate 7 has exactly three relations of which one is never hit (hit / count is a
    multiple of 1/3), predicates 1 and 56 are present."""
    rng = np.random.default_rng(seed)
    gt_masks = np.zeros((nobj, H, W), bool)
    for i in range(nobj):
        y, x = rng.integers(0, H - 16), rng.integers(0, W - 16)
        gt_masks[i, y:y + rng.integers(6, 16), x:x + rng.integers(6, 16)] = True
    gt_labels = rng.integers(1, 134, nobj)
    pairs = [(s, o) for s in range(nobj) for o in range(nobj) if s != o]
    sel = rng.choice(len(pairs), G, replace=False)
    gt_rels = np.array([[pairs[j][0], pairs[j][1], rng.integers(2, 56)] for j in sel])
    unplanted = set()
    if G >= 9:
        gt_rels[gt_rels[:, 2] == 7, 2] = 8
        gt_rels[1] = gt_rels[0]
        gt_rels[2:5, 2] = 7
        gt_rels[5, 2], gt_rels[6, 2] = 1, 56
        unplanted = {1, 3}
    labels = rng.integers(1, 134, 2 * R)
    masks = rng.random((2 * R, H, W)) > 0.97
    rel_dists = rng.random((R, NUM_REL)).astype(np.float32)
    rel_dists[:, 0] = 0
    rows = list(rng.permutation(R))
    for j, (s, o, pr) in enumerate(gt_rels):
        if j in unplanted or (j > 8 and j % 4 == 3):
            continue
        for rep in range(3):                      # hit, wrong predicate, IoU near / below 0.5
            if not rows:
                break
            r = rows.pop()
            labels[r], labels[R + r] = gt_labels[s], gt_labels[o]
            rel_dists[r, pr] = 2.0 if rep != 1 else 0.0
            shift = (0, 1, 4)[rep]
            masks[r] = np.roll(gt_masks[s], shift, axis=1)
            masks[R + r] = np.roll(gt_masks[o], shift, axis=0)
    masks[min(7, R - 1)] = False                  # an empty predicted mask
    rel_pairs = np.stack([np.arange(R), np.arange(R) + R], 1)
    return labels, rel_pairs, rel_dists, masks, gt_rels, gt_labels, gt_masks


def _nan_scene():
    """Two ground-truth objects with EMPTY masks whose classes (133, 132) are carried by three
    predictions each; for 133 the middle one is empty as well (its IoU is 0 / 0, and the next
    value replaces the NaN), for 132 the last one (the NaN is what remains)."""
    labels, rel_pairs, rel_dists, masks, gt_rels, gt_labels, gt_masks = _crafted(9, 100, 9, 7)
    labels[labels >= 132] = 1
    gt_labels[gt_labels >= 132] = 1
    a, b = int(gt_rels[0, 0]), int(gt_rels[0, 1])
    gt_labels[a], gt_labels[b] = 133, 132
    gt_masks[a] = gt_masks[b] = False
    for rows, cls, empty in (((150, 160, 170), 133, 160), ((30, 130, 190), 132, 190)):
        for r in rows:
            labels[r] = cls
            masks[r] = False
            if r != empty:
                masks[r, 5:9, 5:9] = True
    return labels, rel_pairs, rel_dists, masks, gt_rels, gt_labels, gt_masks


def _result(labels, rel_pairs, rel_dists, masks):
    return (None, torch.from_numpy(labels).to(DEV), torch.from_numpy(rel_pairs),
            torch.from_numpy(masks).to(DEV), None, None, None, torch.from_numpy(rel_dists).to(DEV))


@pytest.fixture(scope="module")
def scenes():
    """Per shape: the scene, its device result + device-resident ground-truth masks (as
    `dataset.eval_ground_truth` leaves them), and the oracle's lists (shared, never written)."""
    out = []
    for seed, (R, G, nobj) in enumerate(SHAPES, 1):
        sc = _crafted(seed, R, G, nobj)
        labels, rel_pairs, rel_dists, masks, gt_rels, gt_labels, gt_masks = sc
        ref = OE.evaluate(labels, rel_pairs, rel_dists, masks, gt_rels, gt_labels, gt_masks)
        gt_t, gt_tm = OE.triplets(gt_rels, gt_labels, gt_masks)
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = OE.iou_panseg(gt_t, labels, gt_tm, masks)
        out.append(dict(scene=sc, result=_result(labels, rel_pairs, rel_dists, masks),
                        gt=(gt_rels, gt_labels, torch.from_numpy(gt_masks).to(DEV)),
                        ref=ref, iou=iou))
    torch.cuda.synchronize()
    return out


def _same_records(a, b):
    assert sorted(a) == sorted(b)
    for i in a:
        assert a[i]["G"] == b[i]["G"]
        for k in ("hits", "counts"):
            assert np.array_equal(a[i][k], b[i][k]), (i, k)
        for k in ("sub_iou", "obj_iou"):
            assert np.array_equal(a[i][k], b[i][k], equal_nan=True), (i, k)


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_device_record_equals_the_numpy_record_of_the_oracle_lists(scenes, case):
    from pairnet_amd.evaluation import StreamingEvaluator, host_record
    s = scenes[case]
    R, G, nobj = SHAPES[case]
    gt_rels = s["gt"][0]
    hits, counts = host_record(s["ref"], gt_rels, NUM_REL)
    se = StreamingEvaluator(56)
    se.add(s["result"], *s["gt"], index=5)
    rec = se.records()[5]
    print(SHAPES[case], "hits[:, :, 0] =", rec["hits"][:, :, 0].tolist(), "G =", rec["G"])
    assert rec["G"] == G and rec["hits"].dtype == np.int32
    assert np.array_equal(rec["counts"], counts) and np.array_equal(rec["hits"], hits)
    assert np.array_equal(rec["sub_iou"], s["iou"][0]) and np.array_equal(rec["obj_iou"], s["iou"][1])
    assert len(rec["sub_iou"]) > 0 and hits[0, -1, 0] > 0          # (the planted hits are found)
    if G >= 9:       # the scene has what it was crafted for
        p2g = s["ref"]["pred_to_gt"]
        assert any(0 in l and 1 in l for l in p2g)                 # one prediction, both duplicates
        assert counts[7] == 3 and 0 < hits[0, -1, 7] < 3           # not a dyadic fraction
        assert counts[1] >= 1 and counts[56] >= 1
    if R == 200:     # k = 100 < R: predictions behind row 100 hit what the first 100 do not
        full = len({g for l in s["ref"]["pred_to_gt"] for g in l})
        assert hits[0, 2, 0] < full
        assert hits[0, 0, 0] < hits[0, 1, 0] < hits[0, 2, 0]
    if R == 10:      # every k is above R
        assert (hits[:, 0] == hits[:, 2]).all()


def test_four_images_give_the_host_path_summary(scenes):
    from pairnet_amd.evaluation import SceneGraphMetrics, StreamingEvaluator, TripletEvaluator
    host, ev, se = SceneGraphMetrics(56), TripletEvaluator(), StreamingEvaluator(56)
    for i, s in enumerate(scenes):
        gt_rels, gt_labels, gt_masks = s["gt"]
        host.add(ev(s["result"], gt_rels, gt_labels, gt_masks), gt_rels,
                 iou=ev.iou_stats(s["result"], gt_rels, gt_labels, gt_masks))
        se.add(s["result"], gt_rels, gt_labels, gt_masks)            # (index: the call count)
    se.add(scenes[0]["result"], np.zeros((0, 3), int), *scenes[0]["gt"][1:])
    host.add(ev(scenes[0]["result"], np.zeros((0, 3), int), *scenes[0]["gt"][1:]),
             np.zeros((0, 3), int))
    want, got = host.summary(), se.summary()
    assert got == want
    assert got["images"] == 4 and got["skipped"] == 1 and got["sgdet_mean_recall"][100] > 0
    assert got["subject-IoU"] > 0 and got["phrdet_recall"][100] > 0


def test_iou_walk_keeps_pythons_max_with_nan():
    from pairnet_amd.evaluation import StreamingEvaluator, TripletEvaluator
    labels, rel_pairs, rel_dists, masks, gt_rels, gt_labels, gt_masks = _nan_scene()
    gt_t, gt_tm = OE.triplets(gt_rels, gt_labels, gt_masks)
    with np.errstate(invalid="ignore", divide="ignore"):
        want_s, want_o = OE.iou_panseg(gt_t, labels, gt_tm, masks)
    # relation 0: subject of class 133 (the NaN is replaced: 0.0), object of class 132 (NaN)
    assert want_s[0] == 0.0 and np.isnan(want_o[0]) and not np.isnan(want_o[3:]).any()
    res = _result(labels, rel_pairs, rel_dists, masks)
    se = StreamingEvaluator(56)
    se.add(res, gt_rels, gt_labels, torch.from_numpy(gt_masks).to(DEV))
    rec = se.records()[0]
    assert np.array_equal(rec["sub_iou"], want_s, equal_nan=True)
    assert np.array_equal(rec["obj_iou"], want_o, equal_nan=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        host_s, host_o = TripletEvaluator().iou_stats(res, gt_rels, gt_labels, gt_masks)
    assert np.array_equal(host_s, rec["sub_iou"], equal_nan=True)
    assert np.array_equal(host_o, rec["obj_iou"], equal_nan=True)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_box_records_equal_the_numpy_records_of_the_oracle_lists(seed):
    from pairnet_amd.evaluation import StreamingEvaluator, host_record
    labels, rel_pairs, rel_dists, det, gt_rels, gt_labels, gt_boxes = _box_scene(seed)
    ref = OE.evaluate_boxes(labels, rel_pairs, rel_dists, det[:, :4], gt_rels, gt_labels, gt_boxes)
    result = (torch.from_numpy(det).to(DEV), torch.from_numpy(labels).to(DEV),
              torch.from_numpy(rel_pairs), None, None, torch.from_numpy(rel_dists).to(DEV))
    se = StreamingEvaluator(50)
    se.add_boxes(result, gt_rels, gt_labels, gt_boxes)
    rec = se.records()[0]
    hits, counts = host_record(ref, gt_rels, 51)
    assert np.array_equal(rec["hits"], hits) and np.array_equal(rec["counts"], counts)
    assert hits[0, 2, 0] > 0 and len(rec["sub_iou"]) == 0
    host = StreamingEvaluator(50)
    host.add_host(0, ref, gt_rels)
    assert se.summary() == host.summary()


def test_add_never_waits_for_the_device(scenes, monkeypatch):
    from pairnet_amd.evaluation import StreamingEvaluator, TripletEvaluator
    a, b = scenes[0], scenes[3]
    se = StreamingEvaluator(56)
    se.add(a["result"], *a["gt"])                                   # warm-up
    torch.cuda.synchronize()

    def refuse(name):
        def f(*args, **kw):
            raise AssertionError("host wait: " + name)
        return f
    with monkeypatch.context() as m:
        for name in ("cpu", "item", "numpy", "tolist"):
            m.setattr(torch.Tensor, name, refuse("Tensor." + name))
        with pytest.raises(AssertionError, match="host wait"):      # the check can see a wait
            TripletEvaluator()(b["result"], *b["gt"])
        se.add(b["result"], *b["gt"])
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            TripletEvaluator()(a["result"], *a["gt"])
            flagged = False
        except RuntimeError as e:
            flagged = "synchroniz" in str(e)
            if not flagged:
                raise
        print("set_sync_debug_mode('error') flags the host path:", flagged)
        se.add(scenes[2]["result"], *scenes[2]["gt"])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    one = StreamingEvaluator(56)
    for s in (a, b, scenes[2]):
        one.add(s["result"], *s["gt"])
    _same_records(se.records(), one.records())


def test_images_added_on_two_streams_arrive_whole(scenes):
    from pairnet_amd.evaluation import StreamingEvaluator
    a, b = scenes[3], scenes[0]
    one = StreamingEvaluator(56)
    one.add(a["result"], *a["gt"], index=0)
    one.add(b["result"], *b["gt"], index=1)
    want = one.records()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    se = StreamingEvaluator(56)
    with torch.cuda.stream(s1):
        se.add(a["result"], *a["gt"], index=0)
    with torch.cuda.stream(s2):
        se.add(b["result"], *b["gt"], index=1)
    blob = se.state()                              # (no synchronisation in between)
    _same_records(se.records(), want)
    assert blob.tobytes() == one.state().tobytes()
    torch.cuda.synchronize()


def test_detector_loop_returns_the_host_path_metrics():
    """`multi_gpu_test` with the real detector at 160 x 224 over 5 images, one of them without
    relations; the ground truth is cut from the detector's own results (three of its triplets:
    their masks, labels and predicates), so matches exist."""
    from oracle.backbone import seeded_backbone_state
    from pairnet_amd import build_detector, pairnet_r50
    from pairnet_amd.dist import multi_gpu_test
    from pairnet_amd.evaluation import SceneGraphMetrics, StreamingEvaluator, TripletEvaluator
    det = build_detector(pairnet_r50())
    det.backbone.load_state_dict(seeded_backbone_state(41))
    det.bbox_head.init_weights(seed=3)
    det.to(DEV)
    H, W, N = 160, 224, 5
    metas = [dict(img_shape=(H, W, 3), scale_factor=[2.0] * 4)]
    g = torch.Generator().manual_seed(3)
    data = [(torch.randn(1, 3, H, W, generator=g).to(DEV), metas) for _ in range(N)]
    head, ann = det.bbox_head, []
    R = head.num_rel_query
    for i, (img, m) in enumerate(data):
        res = head.simple_test(det.extract_feat(img), m)[0]
        rows = [0, R, 1, R + 1, 2, R + 2]
        pred = 1 + res[7][:3, 1:].argmax(1).cpu().numpy()
        rels = np.array([[0, 1, pred[0]], [2, 3, pred[1]], [4, 5, pred[2]]])
        ann.append(dict(gt_rels=rels if i != 2 else np.zeros((0, 3), np.int64),
                        gt_labels=res[1][rows].cpu().numpy(), gt_masks=res[3][rows].clone()))
    torch.cuda.synchronize()
    host = multi_gpu_test(det, data, annotations=ann, evaluator=TripletEvaluator(),
                          metrics=SceneGraphMetrics(56), depth=3, calibrate=False)
    se = StreamingEvaluator(56)
    out = multi_gpu_test(det, data, annotations=ann, evaluator=se, depth=3, calibrate=False)
    print("metrics:", {k: out["metrics"][k] for k in ("images", "skipped", "sgdet_recall")})
    assert out["metrics"] == host["metrics"]
    assert out["metrics"]["images"] == 4 and out["metrics"]["skipped"] == 1
    assert torch.equal(out["records"], host["records"])
    assert sorted(se.records()) == [0, 1, 3, 4]
