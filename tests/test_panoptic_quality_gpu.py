"""GPU: `PanopticQuality.add` on the MI355X -- the confusion table, the (tp, fp, fn) record and
the float64 IoU sums csrc/panoptic_quality.hip leaves on the device equal the numpy restatement
`add_host` (itself pinned by tests/pq_ref.py on the CPU) on the same inputs: tables and counts
as integers, IoU sums bitwise; twice the same inputs give the same bits, and so does the
one-add-per-pixel form of the pass."""
import numpy as np
import pytest
import torch

from pq_scenes import NC, OFFSET, make_scene, rgb_of
from test_panoptic_quality import A_GT, A_PRED, A_SEG, B_GT, B_PRED, B_SEG, HAND, P, V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the (G + 1) x 257 table is kept in LDS up to G = 61 (hip.PQ_LDS_MAX_G); from G = 62 on the adds
# go to global memory
G_CASES = (0, 1, 61, 62, 63, 64, 255)


def _compare(sc, nc=NC, things=80):
    """add (twice, and once in the one-add-per-pixel form) against add_host; returns the record."""
    from pairnet_amd import hip
    from pairnet_amd.evaluation import PanopticQuality
    dev_pq = PanopticQuality(nc, things, keep_confusion=True)
    host_pq = PanopticQuality(nc, things, keep_confusion=True)
    pred = torch.from_numpy(np.ascontiguousarray(sc["pred"]).astype(np.int64)).to(DEV)
    rgb = torch.from_numpy(np.ascontiguousarray(sc["rgb"])).to(DEV)
    dev_pq.add(pred, rgb, sc["segments"], index=0)
    dev_pq.add(pred, rgb, sc["segments"], index=1)
    dev_pq.add(pred, rgb, sc["segments"], index=2, flags=hip.PQ_PLAIN)
    host_pq.add_host(0, sc["pred"], sc["gt_id"], sc["segments"])
    d, h = dev_pq.records(), host_pq.records()[0]
    G = len(sc["segments"])
    assert d[0]["N"].shape == (G + 1, 257) and d[0]["N"].dtype == np.int32
    assert int(d[0]["N"].sum()) == sc["pred"].size
    for i in (0, 1, 2):
        assert d[i]["status"] == h["status"] == 0, i
        assert np.array_equal(d[i]["N"], h["N"]), i
        assert np.array_equal(d[i]["rec"], h["rec"]), i
        assert d[i]["iou"].tobytes() == h["iou"].tobytes(), i
    return h


def _flat(H, W, values, ids, cats=(3, 100)):
    """A map whose pixel (y, x) takes entry (y + x) % len(values): one value = one segment over
    the whole map, two = a checkerboard (no runs of equal keys at all)."""
    yy, xx = np.mgrid[0:H, 0:W]
    k = (yy + xx) % len(values)
    gt_id = np.asarray(ids, np.int64)[k]
    seg = [(int(i), cats[j % 2], 0) for j, i in enumerate(sorted(set(ids)))]
    return dict(pred=np.asarray(values, np.int64)[k], gt_id=gt_id, rgb=rgb_of(gt_id),
                segments=np.array(seg, np.int64).reshape(-1, 3))


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (13, 21), (37, 53)])
def test_small_shapes(shape):
    """1 x 7: the last group of four pixels is partial, its RGB dwords would straddle the end;
    13 x 21 = 273 and 37 x 53 = 1961 pixels: no multiple of 4, of 256 or of 2048."""
    H, W = shape
    h = _compare(make_scene(5, H, W, 9, perturb=H * W > 7))
    if H * W > 7:
        assert h["rec"][:, 0].sum() > 0 and h["rec"][:, 1].sum() > 0


@pytest.mark.parametrize("G", G_CASES)
def test_table_in_lds_and_in_global_memory(G):
    h = _compare(make_scene(40 + G, 37, 53, G))
    if G >= 8:
        assert h["rec"][:, 0].sum() > 0 and h["rec"][:, 2].sum() > 0
    if G == 255:                                    # region 255 -> segment 0, region 0 -> 255
        assert h["N"][:, 0].sum() > 0 and h["N"][:, 255].sum() > 0


def test_one_segment_and_checkerboard():
    # every lane of every wavefront in ONE bin (the aggregated add), segment 255
    h = _compare(_flat(37, 53, [P(255, 3)], [0xABCDEF]))
    assert h["N"][1, 255] == 37 * 53 and h["rec"][3].tolist() == [1, 0, 0] and h["iou"][3] == 1.0
    # two segments (0 and 255) alternating pixel by pixel: no two neighbours share a key
    h = _compare(_flat(37, 53, [P(0, 3), P(255, 100)], [1, 0xFFFFFF]))
    assert h["rec"][3].tolist() == [1, 0, 0] and h["rec"][100].tolist() == [1, 0, 0]
    # the same prediction against a ground truth of period 3: every pair overlaps, none matches
    sc = _flat(37, 53, [P(0, 3), P(255, 100)], [1, 0xFFFFFF])
    sc["gt_id"] = np.array([1, 0xFFFFFF, 0])[(np.mgrid[0:37, 0:53].sum(0)) % 3]
    sc["rgb"] = rgb_of(sc["gt_id"])
    h = _compare(sc)
    assert h["rec"][:, 0].sum() == 0 and (h["N"][:, [0, 255]] > 0).all()


def test_ground_truth_ids_at_the_24_bit_extremes():
    """ids 1 and 0xFFFFFF, and ids that differ in the blue (highest) byte only."""
    ids = [1, 0x000203, 0x010203, 0x020203, 0xFE0203, 0xFF0203, 0xFFFFFE, 0xFFFFFF, 0x010000,
           0x0000FF, 0x00FF00]
    sc = make_scene(3, 37, 53, 10, ids=ids)
    assert set(np.unique(sc["gt_id"]).tolist()) == set(ids) | {0}
    h = _compare(sc)
    assert h["rec"][:, 0].sum() > 0 and (h["N"][1:].sum(1) > 0).all()


def test_hand_made_maps_of_the_cpu_file():
    """The crowd, void and exact-1/2 cases, with their worked answers."""
    for pred, gt, seg, want, iou in HAND:
        seg = np.array(seg, np.int64).reshape(-1, 3)
        h = _compare(dict(pred=pred, gt_id=gt, rgb=rgb_of(gt), segments=seg), 5, 3)
        assert h["rec"].tolist() == want and h["iou"].tolist() == iou
    gt = A_GT.copy()
    gt[3, 0] = 20
    h = _compare(dict(pred=A_PRED, gt_id=gt, rgb=rgb_of(gt), segments=np.array(A_SEG)), 5, 3)
    assert h["rec"][1].tolist() == [2, 0, 0]
    gt = B_GT.copy()
    gt[0, 2] = 0
    h = _compare(dict(pred=B_PRED, gt_id=gt, rgb=rgb_of(gt), segments=np.array(B_SEG)), 5, 3)
    assert h["rec"][0].tolist() == [0, 0, 0]


@pytest.fixture(scope="module")
def large():
    """800 x 1333, 40 ground-truth segments, 60 predicted ones (42 regions, one merged away, one
    dropped, 20 split)."""
    sc = make_scene(11, 800, 1333, 40, split=20)
    assert len(np.unique(sc["pred"])) == 61                 # 60 segments + void
    return sc


def test_production_size(large):
    h = _compare(large)
    print("800 x 1333: tp %d fp %d fn %d" % tuple(h["rec"].sum(0)))
    assert h["rec"][:, 0].sum() >= 20 and h["rec"][:, 1].sum() > 0 and h["rec"][:, 2].sum() > 0


def test_status_flags_reach_the_summary(large):
    from pairnet_amd import evaluation as E
    pred = torch.from_numpy(large["pred"]).to(DEV)
    rgb = torch.from_numpy(large["rgb"]).to(DEV)
    for y, x, bad, bit in ((0, 0, P(256, 3), E.PQ_BAD_SEGMENT), (799, 1332, P(7, 134), E.PQ_BAD_VALUE),
                           (400, 5, -1, E.PQ_BAD_VALUE), (13, 700, None, E.PQ_TWO_CATEGORIES)):
        p = pred.clone()
        v = int(large["pred"][y, x])
        assert v % OFFSET != NC                              # (a segment pixel)
        p[y, x] = bad if bad is not None else v - v % OFFSET + (v % OFFSET + 1) % NC
        pq = E.PanopticQuality()
        pq.add(pred, rgb, large["segments"], index=3)
        pq.add(p, rgb, large["segments"], index=8)
        host = E.PanopticQuality()
        host.add_host(8, p.cpu(), large["gt_id"], large["segments"])
        rec = pq.records()
        assert rec[3]["status"] == 0 and rec[8]["status"] == bit == host.records()[8]["status"]
        with pytest.raises(ValueError, match="image 8 "):
            pq.summary()
    with pytest.raises(ValueError, match="differ in size"):   # before anything is enqueued
        pq.add(pred[:-1], rgb, large["segments"], index=9)
    assert 9 not in pq.records()


def test_add_on_a_side_stream_summary_from_the_default_stream(large):
    from pairnet_amd.evaluation import PanopticQuality
    small = make_scene(2, 37, 53, 9)
    want = PanopticQuality()
    want.add_host(0, large["pred"], large["gt_id"], large["segments"])
    want.add_host(1, small["pred"], small["gt_id"], small["segments"])
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    pq = PanopticQuality()
    with torch.cuda.stream(s1):
        pq.add(torch.from_numpy(large["pred"]).to(DEV, non_blocking=True), large["rgb"],
               large["segments"], index=0)                  # (host PNG: pinned, non-blocking)
    with torch.cuda.stream(s2):
        pq.add(torch.from_numpy(small["pred"]).to(DEV), torch.from_numpy(small["rgb"]).to(DEV),
               small["segments"], index=1)
    got = pq.summary()                                      # (no synchronisation in between)
    assert got == want.summary() and got["images"] == 2
    assert pq.state().tobytes() == want.state().tobytes()
    torch.cuda.synchronize()


def test_add_never_waits_for_the_device(large):
    from pairnet_amd.evaluation import PanopticQuality
    pred = torch.from_numpy(large["pred"]).to(DEV)
    rgb = torch.from_numpy(large["rgb"]).to(DEV)
    pq = PanopticQuality()
    pq.add(pred, rgb, large["segments"])                    # warm-up
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pq.add(pred, rgb, large["segments"])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    rec = pq.records()
    assert np.array_equal(rec[0]["rec"], rec[1]["rec"])


def test_panoptic_map_of_the_head():
    """`add(result[4], ...)` on the map `CrossHead2.get_bboxes` writes (seeded detector, 160 x
    224), against `add_host(result[4].cpu(), ...)`; the ground truth is cut from the map itself
    (one segment per predicted value, shifted by two pixels), so matches exist."""
    from oracle.backbone import seeded_backbone_state
    from pairnet_amd import build_detector, pairnet_r50
    from pairnet_amd.evaluation import PanopticQuality
    det = build_detector(pairnet_r50())
    det.backbone.load_state_dict(seeded_backbone_state(41))
    det.bbox_head.init_weights(seed=3)
    det.to(DEV)
    H, W = 160, 224
    metas = [dict(img_shape=(H, W, 3), scale_factor=[2.0] * 4)]
    img = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(3)).to(DEV)
    res = det.bbox_head.simple_test(det.extract_feat(img), metas)[0]
    pan = res[4]
    assert pan.dtype == torch.int64 and pan.dim() == 2 and pan.is_cuda
    host = pan.cpu().numpy()
    values = [int(v) for v in np.unique(host) if v % OFFSET != NC]
    ids = {v: 1000 + 7 * i for i, v in enumerate(values)}
    gt_id = np.zeros_like(host)
    for v, i in ids.items():
        gt_id[host == v] = i
    gt_id = np.roll(gt_id, 2, 1)
    seg = np.array([(i, v % OFFSET, 0) for v, i in ids.items()], np.int64).reshape(-1, 3)
    dev_pq, host_pq = PanopticQuality(keep_confusion=True), PanopticQuality(keep_confusion=True)
    dev_pq.add(res, torch.from_numpy(rgb_of(gt_id)).to(DEV), seg)      # (the 8-tuple itself)
    host_pq.add_host(0, pan.cpu(), gt_id, seg)
    d, h = dev_pq.records()[0], host_pq.records()[0]
    print("map %s: %d segments, tp %d fp %d fn %d" % ((tuple(host.shape), len(values))
                                                      + tuple(h["rec"].sum(0))))
    assert d["status"] == h["status"] == 0 and np.array_equal(d["N"], h["N"])
    assert np.array_equal(d["rec"], h["rec"]) and d["iou"].tobytes() == h["iou"].tobytes()
    assert dev_pq.summary() == host_pq.summary()
