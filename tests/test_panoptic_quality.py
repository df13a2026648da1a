"""CPU: `pairnet_amd.evaluation.PanopticQuality` -- the per-image record in its numpy form
(`add_host`: the restatement csrc/panoptic_quality.hip is tested against on the GPU,
tests/test_panoptic_quality_gpu.py) on hand-made maps with worked answers and against the
independent slow statement tests/pq_ref.py; the summary, state / merge, the status flags, the
loop's new keyword, and the two C entries (refusals, declarations, compile report)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pq_ref
from pq_scenes import NC, OFFSET, make_scene, rgb_of
from test_streaming_eval import _HostDetector, _host_annotations, _host_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 5                                    # the hand-made maps use 5 classes: value 5 is void


def _pq(nc=5, things=3, **kw):
    from pairnet_amd.evaluation import PanopticQuality
    return PanopticQuality(num_classes=nc, num_things=things, **kw)


def P(s, c):
    return s * OFFSET + c


# ---- hand-made map A, 4 x 6: an exact match, iou exactly 1/2, iou 2/3 -------------------------
# ground truth (ids)                 prediction (segment:class)
#   10 10 10 10 10 10                  1:0 1:0 1:0 1:0 1:0 1:0
#   10 10 10 10 10 10                  1:0 1:0 1:0 1:0 1:0 1:0
#   20 30 40 40 30 30                  2:1 4:2 3:1 3:1 3:1 4:2
#   30 30 30 30 30 30                  2:1 4:2 4:2 4:2 4:2 4:2
# table: 10 -> class 0, 20 -> 1, 30 -> 2, 40 -> 1 (none crowd)
#   10 x seg 1: N = 12, union = 12 + 12 - 12 = 12: iou 1            -> tp[0], iou[0] = 1
#   20 x seg 2: N = 1, union = 2 + 1 - 1 = 2: 2 N = union, iou = 1/2 exactly: NOT matched
#               -> fn[1] (id 20), fp[1] (seg 2; no void, no crowd under it)
#   40 x seg 3: N = 2, union = 3 + 2 - 2 = 3: 2 N = 4 > 3            -> tp[1], iou[1] = 2/3
#   30 x seg 4: N = 7, union = 7 + 9 - 7 = 9: 14 > 9                 -> tp[2], iou[2] = 7/9
A_GT = np.array([[10] * 6, [10] * 6, [20, 30, 40, 40, 30, 30], [30] * 6])
A_PRED = np.array([[P(1, 0)] * 6, [P(1, 0)] * 6,
                   [P(2, 1), P(4, 2), P(3, 1), P(3, 1), P(3, 1), P(4, 2)],
                   [P(2, 1)] + [P(4, 2)] * 5])
A_SEG = [(10, 0, 0), (20, 1, 0), (30, 2, 0), (40, 1, 0)]
A_REC = [[1, 0, 0], [1, 1, 1], [1, 0, 0], [0, 0, 0], [0, 0, 0]]
A_IOU = [1.0, 2 / 3, 7 / 9, 0.0, 0.0]

# ---- hand-made map B, 6 x 6: void, an unlisted id, crowds, the void prediction ----------------
#   0  0 10 10 99 99                   1:0 1:0 1:0 1:0 2:0 2:0
#  99 10 10 10 10 10                   2:0 2:0  V   V   V   V
#  20 20 20 20 10 10                   3:3 3:3 3:3 3:3  V   V
#  30 30 30 30 10 10                   4:4 4:4 4:4 4:4  V   V
#  10 10 10 10 10 10                    V   V   V   V   V   V
#  10 10 10 10 10 10                    V   V   V   V   V   V
# table: 10 -> class 1; 20 -> class 3, crowd; 30 -> class 3, crowd.  99 is not listed: void.
#   seg 1 (class 0, 4 px): 2 on void: 2 * 2 = 4 = area, fraction exactly 1/2: COUNTED -> fp[0]
#   seg 2 (class 0, 4 px): 3 on the unlisted id = void: 6 > 4: absorbed, not counted
#   seg 3 (class 3, 4 px): on crowd 20 of class 3: 8 > 4: absorbed, not counted
#   seg 4 (class 4, 4 px): on crowd 30 of class 3, another class: nothing absorbs it -> fp[4]
#   10 is never matched (seg 1 / 2 have class 0) -> fn[1]; crowds 20 / 30 are never fn
B_GT = np.array([[0, 0, 10, 10, 99, 99], [99, 10, 10, 10, 10, 10], [20] * 4 + [10] * 2,
                 [30] * 4 + [10] * 2, [10] * 6, [10] * 6])
B_PRED = np.array([[P(1, 0)] * 4 + [P(2, 0)] * 2, [P(2, 0)] * 2 + [V] * 4, [P(3, 3)] * 4 + [V] * 2,
                   [P(4, 4)] * 4 + [V] * 2, [V] * 6, [V] * 6])
B_SEG = [(10, 1, 0), (20, 3, 1), (30, 3, 1)]
B_REC = [[0, 1, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 1, 0]]

# ---- C: no ground-truth segment at all (every pixel void): nothing is counted ------------------
C_GT = np.array([[0, 0, 7, 7, 7, 7]] * 4)
C_PRED = np.array([[P(0, 0)] * 3 + [V] * 3] * 4)
# ---- D: ground truth, only void predictions: 10 (class 1) -> fn[1]; the crowd 20 is not ---------
D_GT = np.array([[10, 10, 10, 20, 20, 20]] * 4)
D_PRED = np.full((4, 6), V)
D_SEG = [(20, 2, 1), (10, 1, 0)]           # (unsorted on purpose)
D_REC = [[0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]]

HAND = [(A_PRED, A_GT, A_SEG, A_REC, A_IOU), (B_PRED, B_GT, B_SEG, B_REC, [0.0] * 5),
        (C_PRED, C_GT, [], [[0, 0, 0]] * 5, [0.0] * 5), (D_PRED, D_GT, D_SEG, D_REC, [0.0] * 5)]


def _hand(order=range(4), **kw):
    pq = _pq(**kw)
    for i in order:
        pq.add_host(i, *HAND[i][:3])
    return pq


def test_hand_made_maps_give_the_worked_answers():
    rec = _hand().records()
    for i, (pred, gt, seg, want, iou) in enumerate(HAND):
        assert rec[i]["status"] == 0
        assert rec[i]["rec"].tolist() == want, i
        assert rec[i]["iou"].tolist() == iou, i
        assert rec[i]["rec"].dtype == np.int32 and rec[i]["iou"].dtype == np.float64
        ref = pq_ref.dense(pq_ref.image_record(pred, gt, seg, 5, OFFSET), 5)
        assert ref[0].tolist() == want and ref[1].tolist() == iou, i
    # one pixel of map A's pair at exactly 1/2 moved: (3, 0) from 30 to 20 -> N = 2, union = 2
    gt = A_GT.copy()
    gt[3, 0] = 20
    pq = _pq()
    pq.add_host(0, A_PRED, gt, A_SEG)
    r = pq.records()[0]
    assert r["rec"][1].tolist() == [2, 0, 0] and r["iou"][1] == 2 / 3 + 1.0
    # map B's segment 1 with three of its four pixels on void: absorbed
    gt = B_GT.copy()
    gt[0, 2] = 0
    pq = _pq()
    pq.add_host(0, B_PRED, gt, B_SEG)
    assert pq.records()[0]["rec"][0].tolist() == [0, 0, 0]


def test_hand_made_summary():
    # tp = [1, 1, 1, 0, 0], fp = [1, 1, 0, 0, 1], fn = [0, 3, 0, 0, 0], iou = [1, 2/3, 7/9]:
    #   class 0: pq = 1 / 1.5, sq = 1, rq = 1 / 1.5;  class 1: pq = (2/3) / 3, sq = 2/3, rq = 1/3
    #   class 2: pq = sq = 7/9, rq = 1;  class 3: no sample, excluded;  class 4: fp only: zeros
    s = _hand().summary()
    cw = {0: (1 / 1.5, 1.0, 1 / 1.5), 1: ((2 / 3) / 3.0, 2 / 3, 1 / 3.0), 2: (7 / 9, 7 / 9, 1.0),
          4: (0.0, 0.0, 0.0)}
    assert s["classwise"] == cw and s["images"] == 4
    assert s["n"] == dict(all=4, things=3, stuff=1)          # things: classes < 3
    for j, k in enumerate(("PQ", "SQ", "RQ")):
        assert s[k] == 100.0 * ((cw[0][j] + cw[1][j] + cw[2][j] + cw[4][j]) / 4)
        assert s[k + "_th"] == 100.0 * ((cw[0][j] + cw[1][j] + cw[2][j]) / 3)
        assert s[k + "_st"] == 0.0 and isinstance(s[k], float)
    assert s == pq_ref.summarize([pq_ref.image_record(p, g, sg, 5, OFFSET)
                                  for p, g, sg, _, _ in HAND], 5, 3)
    assert _pq().summary()["PQ"] == 0.0                      # nothing added


# ---- add_host against the independent statement -------------------------------------------------
SEEDS = tuple(range(1, 21))


@pytest.fixture(scope="module")
def scenes():
    out = []
    for seed in SEEDS:
        sc = make_scene(seed, 37, 53, 8 + seed % 4, split=1 + seed % 2)
        sc["ref"] = pq_ref.image_record(sc["pred"], sc["gt_id"], sc["segments"], NC, OFFSET)
        out.append(sc)
    return out


def test_reference_records_cover_every_outcome(scenes):
    """(about the test's own inputs: a matcher that never matches, or never absorbs, fails below)"""
    tot = {k: sum(sum(s["ref"][k].values()) for s in scenes) for k in ("tp", "fp", "fn")}
    tot.update({k: sum(s["ref"][k] for s in scenes) for k in ("void_absorbed", "crowd_absorbed")})
    print(tot)
    assert all(v >= 5 for v in tot.values()), tot
    assert all(sum(s["ref"]["tp"].values()) > 0 for s in scenes)


def test_add_host_equals_the_slow_statement(scenes):
    from pairnet_amd.evaluation import PanopticQuality
    pq = PanopticQuality(keep_confusion=True)
    for i, s in enumerate(scenes):
        pq.add_host(i, s["pred"], s["gt_id"], s["segments"])
    rec = pq.records()
    for i, s in enumerate(scenes):
        ints, iou = pq_ref.dense(s["ref"], NC)
        assert rec[i]["status"] == 0
        assert np.array_equal(rec[i]["rec"], ints), i
        assert rec[i]["iou"].tobytes() == iou.tobytes(), i
        assert np.array_equal(rec[i]["N"], pq_ref.dense_table(s["ref"], s["segments"],
                                                              len(s["segments"]))), i
    assert pq.summary() == pq_ref.summarize([s["ref"] for s in scenes])
    s = pq.summary()
    assert s["n"]["things"] == 3 and s["n"]["stuff"] == 3 and 0 < s["PQ"] < 100   # split at 80


def test_states_merge_in_any_order_to_the_single_run(scenes):
    from pairnet_amd.evaluation import PanopticQuality

    def run(idx):
        pq = PanopticQuality()
        for i in idx:
            pq.add_host(i, scenes[i]["pred"], scenes[i]["gt_id"], scenes[i]["segments"])
        return pq
    n = len(scenes)
    one = run(range(n))
    want = one.summary()
    assert run(reversed(range(n))).summary() == want
    parts = [run(range(r, n, 3)).state() for r in range(3)]
    assert all(b.dtype == np.float64 and b.ndim == 1 for b in parts)
    for order in ((0, 1, 2), (2, 0, 1)):
        m = PanopticQuality()
        m.merge([parts[j] for j in order])
        assert m.summary() == want and m.state().tobytes() == one.state().tobytes()
    with pytest.raises(ValueError, match="twice"):
        PanopticQuality().merge([parts[0], parts[0]])
    for other in (PanopticQuality(num_classes=100), PanopticQuality(num_things=81),
                  PanopticQuality(instance_offset=2000)):
        with pytest.raises(ValueError, match="configuration"):
            other.merge(parts)
    with pytest.raises(ValueError, match="configuration"):
        PanopticQuality().merge([parts[0][:-1]])
    with pytest.raises(ValueError, match="added before"):
        one.add_host(0, scenes[0]["pred"], scenes[0]["gt_id"], scenes[0]["segments"])


def test_status_flags_raise_in_summary_naming_the_image():
    from pairnet_amd import evaluation as E
    for bad, bit, word in ((P(256, 0), E.PQ_BAD_SEGMENT, "256"), (P(1, 6), E.PQ_BAD_VALUE, "class"),
                           (P(1, 2), E.PQ_TWO_CATEGORIES, "two classes")):
        pred = A_PRED.copy()
        pred[0, 0] = bad                   # (segment 1 has class 0 elsewhere)
        pq = _pq()
        pq.add_host(0, A_PRED, A_GT, A_SEG)
        pq.add_host(17, pred, A_GT, A_SEG)
        assert pq.records()[17]["status"] == bit and pq.records()[0]["status"] == 0
        with pytest.raises(ValueError, match="image 17 .*" + word):
            pq.summary()
        m = _pq()
        m.merge([pq.state()])              # the flag travels in the blob
        with pytest.raises(ValueError, match="image 17"):
            m.summary()


def test_bad_inputs_are_refused_on_the_host():
    pq = _pq()
    with pytest.raises(ValueError, match="differ in size"):
        pq.add_host(0, A_PRED, B_GT, A_SEG)
    for seg in ([(10, 5, 0)], [(10, 0, 0), (10, 1, 0)], [(0, 0, 0)], [(1 << 24, 0, 0)],
                [(i + 1, 0, 0) for i in range(256)]):
        with pytest.raises(ValueError, match="gt_segments|255"):
            pq.add_host(0, A_PRED, A_GT, seg)
    assert pq.summary()["images"] == 0
    from pairnet_amd.evaluation import PanopticQuality
    for kw in (dict(num_classes=1000), dict(num_classes=0), dict(num_things=134),
               dict(instance_offset=133)):
        with pytest.raises(ValueError):
            PanopticQuality(**kw)
    from pairnet_amd import head
    assert PanopticQuality().instance_offset == head.INSTANCE_OFFSET


def test_panoptic_ground_truth_keeps_iscrowd_and_sorts():
    from pairnet_amd import dataset
    d = dict(segments_info=[dict(id=300, category_id=7, iscrowd=1, isthing=1),
                            dict(id=20, category_id=90, iscrowd=0, isthing=0)])
    gt = dataset.panoptic_ground_truth(d, rgb_of(np.array([[20, 300], [0, 20]])), "cpu")
    assert gt["gt_segments"].tolist() == [[20, 90, 0], [300, 7, 1]]
    assert tuple(gt["gt_pan"].shape) == (2, 2, 3) and gt["gt_pan"].dtype == torch.uint8
    from pairnet_amd.evaluation import rgb2id
    assert rgb2id(gt["gt_pan"].numpy()).tolist() == [[20, 300], [0, 20]]
    assert rgb2id(np.array([[[1, 2, 3]]], np.uint8)).tolist() == [[1 + 2 * 256 + 3 * 65536]]


# ---- the loop ------------------------------------------------------------------------------------
def _host_panoptic():
    from pairnet_amd.evaluation import PanopticQuality

    class _HostPanoptic(PanopticQuality):
        """`add` through `add_host`: the loop needs `add`, `state`, `merge` and `summary`."""
        seen = []

        def add(self, pan_seg, gt_pan_rgb, gt_segments, index=None):
            from pairnet_amd.evaluation import rgb2id
            self.seen.append(index)
            self.add_host(index, pan_seg, rgb2id(gt_pan_rgb), gt_segments)
    return _HostPanoptic(num_classes=5, num_things=3)


class _PanDetector(_HostDetector):
    @staticmethod
    def detect(img):
        res, sub, obj = _HostDetector.detect(img)
        i = int(img.flatten()[0])
        return res[:4] + (torch.from_numpy(HAND[i % 4][0]),) + res[5:], sub, obj


def test_loop_scores_the_panoptic_maps_with_the_new_keyword():
    from pairnet_amd.dist import multi_gpu_test
    n = 5
    ann = _host_annotations(n)
    for i in (0, 1, 3, 4):                 # image 2 carries no panoptic ground truth
        ann[i].update(gt_pan=rgb_of(HAND[i % 4][1]), gt_segments=HAND[i % 4][2])
    pq = _host_panoptic()
    out = multi_gpu_test(_PanDetector(), _host_dataset(n), annotations=ann, panoptic=pq, depth=2)
    want = _pq()
    for i in (0, 1, 3, 4):
        want.add_host(i, *HAND[i % 4][:3])
    assert out["panoptic"] == want.summary() and out["panoptic"]["images"] == 4
    assert sorted(pq.seen) == [0, 1, 3, 4] and "metrics" not in out
    # without the keyword nothing changes
    plain = multi_gpu_test(_PanDetector(), _host_dataset(n), annotations=ann, depth=2)
    assert "panoptic" not in plain and torch.equal(plain["records"], out["records"])


# ---- the C entries -------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_launching(built_lib):
    from pairnet_amd import hip
    lib = hip.lib()
    p = 4096                                                 # (never dereferenced: refused first)
    ok = dict(pred=p, rgb=p, H=800, W=1333, ids=p, G=40, nc=133, off=1000, fl=0, N=p, cat=p, st=p)

    def confusion(**kw):
        a = dict(ok, **kw)
        return lib.pn_pq_confusion(a["pred"], a["rgb"], a["H"], a["W"], a["ids"], a["G"], a["nc"],
                                   a["off"], a["fl"], a["N"], a["cat"], a["st"], None)
    for k in ("pred", "rgb", "ids", "N", "cat", "st"):
        assert confusion(**{k: None}) == -1, k
    for kw in (dict(H=0), dict(W=0), dict(H=-1), dict(H=46341, W=46341), dict(H=1 << 16, W=1 << 15),
               dict(G=-1), dict(G=256), dict(nc=0), dict(nc=1000), dict(off=133), dict(fl=2),
               dict(pred=p + 8), dict(rgb=p + 2)):
        assert confusion(**kw) == -1, kw
    ok = dict(N=p, cat=p, gc=p, gk=p, G=40, nc=133, ag=p, ap=p, m=p, rec=p, iou=p, st=p)

    def record(**kw):
        a = dict(ok, **kw)
        return lib.pn_pq_record(a["N"], a["cat"], a["gc"], a["gk"], a["G"], a["nc"], a["ag"],
                                a["ap"], a["m"], a["rec"], a["iou"], a["st"], None)
    for k in ("N", "cat", "gc", "gk", "ag", "ap", "m", "rec", "iou", "st"):
        assert record(**{k: None}) == -1, k
    for kw in (dict(G=-1), dict(G=256), dict(nc=0), dict(nc=1000)):
        assert record(**kw) == -1, kw


def test_header_bindings_and_exports_are_consistent():
    import pairnet_amd
    from pairnet_amd import build as B
    from pairnet_amd import hip
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    for name in ("pn_pq_confusion", "pn_pq_record"):
        assert name in declared and name in hip._SIGS and name in hip.EXPORTS, name
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION == 34
    assert callable(hip.pq_confusion) and callable(hip.pq_record)
    assert "panoptic_quality" in B.SOURCES
    for cite in ("psg.py:309-335", "pairnet_head.py:882", "INTEGRATION.md 3a-2"):
        assert cite in header, cite
    assert int(re.search(r"#define PN_PQ_PLAIN (\d+)", header).group(1)) == hip.PQ_PLAIN
    assert pairnet_amd.PanopticQuality is pairnet_amd.evaluation.PanopticQuality
    assert "PanopticQuality" in pairnet_amd.api.__all__
    # the LDS table: 256 column categories + G ids + (G + 1) * 257 bins, 64 KB a workgroup
    src = open(os.path.join(B.CSRC, "panoptic_quality.hip")).read()
    assert int(re.search(r"#define PQ_LDS_MAX_G (\d+)", src).group(1)) == hip.PQ_LDS_MAX_G
    lds = lambda G: 4 * (256 + G + (G + 1) * hip.PQ_COLS)
    assert lds(hip.PQ_LDS_MAX_G) <= 65536 < lds(hip.PQ_LDS_MAX_G + 1)


def test_panoptic_kernels_compile_for_gfx950_without_scratch(tmp_path):
    from pairnet_amd import build as B
    out = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(B.CSRC, "panoptic_quality.hip"),
                          "-o", str(tmp_path / "panoptic_quality.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+(.*)", line)
        if not m:
            continue
        f = re.match(r"Function Name: (\S+)", m.group(1))
        if f:
            cur = res.setdefault(f.group(1), {})
            continue
        kv = re.match(r"(.+?): (\d+)", m.group(1))
        if kv and cur is not None:
            cur[kv.group(1).strip()] = int(kv.group(2))
    kernels = {k: v for k, v in res.items() if "k_pq_" in k}
    # the initialisation, four forms of the pass over the pixels, the record
    assert len(kernels) == 6 and sum("k_pq_confusion" in k for k in kernels) == 4, sorted(res)
    for k, use in kernels.items():
        print(k, use)
        assert use["ScratchSize [bytes/lane]"] == 0, k
        # static LDS; the pass over the pixels adds its dynamic table, bounded in the test above
        assert use["LDS Size [bytes/block]"] <= 65536, k
