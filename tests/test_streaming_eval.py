"""CPU: `pairnet_amd.evaluation.StreamingEvaluator` -- the per-image integer record (here in
its numpy form, `add_host` / `host_record`: the restatement csrc/evaluate.hip is tested against
on the GPU, tests/test_streaming_eval_gpu.py) reproduces the reference-pinned chain
`oracle.evaluation.evaluate` -> `SceneGraphMetrics` exactly; blobs merge across ranks in any
order; `dist.multi_gpu_test` takes the streaming path for an evaluator with `add` and `state`;
the two new C entries refuse bad arguments, are declared, and compile without scratch."""
import os
import re
import socket
import subprocess
import sys
import types
import importlib.util

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import evaluation as OE
from oracle import ref_shim
from test_evaluation import _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_REL = 57


def _images():
    """Seeds 1-4 of the crafted scene plus one image without relations (index 2):
    [(image_eval, gt_rels, (sub_iou, obj_iou))]."""
    out = []
    for seed in (1, 2, None, 3, 4):
        if seed is None:
            out.append((dict(pred_to_gt=[], phrdet_pred_to_gt=[], sgdet_recall=None,
                             phrdet_recall=None), np.zeros((0, 3), int), None))
            continue
        labels, rel_pairs, rel_dists, masks, gt_rels, gt_labels, gt_masks = _scene(seed)
        ev = OE.evaluate(labels, rel_pairs, rel_dists, masks, gt_rels, gt_labels, gt_masks)
        gt_t, gt_tm = OE.triplets(gt_rels, gt_labels, gt_masks)
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = OE.iou_panseg(gt_t, labels, gt_tm, masks)
        out.append((ev, gt_rels, iou))
    return out


@pytest.fixture(scope="module")
def images():
    return _images()


@pytest.fixture(scope="module")
def want(images):
    """The existing chain's summary of the same images (shared, never written)."""
    from pairnet_amd.evaluation import SceneGraphMetrics
    agg = SceneGraphMetrics(num_predicates=56)
    for ev, gt_rels, iou in images:
        agg.add(ev, gt_rels, iou=iou)
    return agg.summary()


def _streamed(images, order=None):
    from pairnet_amd.evaluation import StreamingEvaluator
    se = StreamingEvaluator(56)
    for i in (order if order is not None else range(len(images))):
        ev, gt_rels, iou = images[i]
        se.add_host(i, ev, gt_rels, iou=iou)
    return se


def test_host_records_reproduce_the_scene_graph_metrics_chain(images, want):
    se = _streamed(images)
    got = se.summary()
    assert got == want
    assert got["images"] == 4 and got["skipped"] == 1 and got["sgdet_mean_recall"][100] > 0
    assert "subject-IoU" in got and got["subject-IoU"] > 0
    # the record itself: slot 0 counts every relation, the other slots add up to it
    rec = se.records()
    assert sorted(rec) == [0, 1, 3, 4]
    for r in rec.values():
        assert r["counts"][0] == r["G"] == r["counts"][1:].sum()
        assert (r["hits"][:, :, 0] == r["hits"][:, :, 1:].sum(-1)).all()
        assert (r["hits"] <= r["counts"]).all() and r["hits"].dtype == np.int32
    # default index = the call count
    from pairnet_amd.evaluation import StreamingEvaluator
    auto = StreamingEvaluator(56)
    for ev, gt_rels, iou in images:
        auto.add_host(None, ev, gt_rels, iou=iou)
    assert auto.summary() == want
    with pytest.raises(ValueError):
        auto.add_host(0, images[0][0], images[0][1])


@pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")
def test_mean_recall_equals_the_reference_class(images):
    sys.dont_write_bytecode = True
    for name, attrs in (("mmdet", {}), ("mmdet.core", dict(bbox_overlaps=None)),
                        ("terminaltables", dict(AsciiTable=None))):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            if not hasattr(m, k):
                setattr(m, k, v)
    pkg = types.ModuleType("refevals")
    pkg.__path__ = [os.path.join(ref_shim.REF_ROOT, "pairnet/evaluation")]
    sys.modules["refevals"] = pkg
    mods = {}
    for n in ("sgg_eval_util", "sgg_metrics"):
        spec = importlib.util.spec_from_file_location(
            "refevals." + n, os.path.join(ref_shim.REF_ROOT, "pairnet/evaluation", n + ".py"))
        mods[n] = importlib.util.module_from_spec(spec)
        sys.modules["refevals." + n] = mods[n]
        spec.loader.exec_module(mods[n])
    M = mods["sgg_metrics"]
    mr = M.SGMeanRecall({}, {}, [], NUM_REL, ["bg"] + ["p%d" % i for i in range(1, NUM_REL)],
                        detection_method="pan_seg")
    mr.register_container("sgdet")
    for ev, gt_rels, _ in images:
        if len(gt_rels):
            mr.collect_mean_recall_items({}, dict(pred_to_gt=ev["pred_to_gt"],
                                                  phrdet_pred_to_gt=ev["phrdet_pred_to_gt"],
                                                  gt_rels=gt_rels), "sgdet")
    mr.calculate_mean_recall("sgdet")
    got = _streamed(images).summary()
    for mode in ("sgdet", "phrdet"):
        assert got[mode + "_mean_recall"] == mr.result_dict[mode + "_mean_recall"]
        assert got[mode + "_mean_recall_list"] == mr.result_dict[mode + "_mean_recall_list"]


def test_states_of_two_ranks_merge_to_the_same_summary(images, want):
    from pairnet_amd.evaluation import StreamingEvaluator
    a, b = _streamed(images, (0, 2, 4)), _streamed(images, (1, 3))
    sa, sb = a.state(), b.state()
    assert isinstance(sa, np.ndarray) and sa.dtype == np.float64 and sa.ndim == 1
    for states in ((sa, sb), (sb, sa)):
        m = StreamingEvaluator(56)
        m.merge(list(states))
        assert m.summary() == want
    a.merge([sa, sb])                 # rank 0 merges into itself: its own state is among them
    assert a.summary() == want
    with pytest.raises(ValueError):
        StreamingEvaluator(56).merge([sa, sa])
    with pytest.raises(ValueError):
        StreamingEvaluator(50).merge([sa])
    one = StreamingEvaluator(56)
    one.merge([_streamed(images).state()])
    assert one.summary() == want and one.state().tobytes() == _streamed(images).state().tobytes()


def test_order_of_adding_does_not_matter(images, want):
    assert _streamed(images, (3, 0, 4, 2, 1)).summary() == want


# ---- the loop (stand-ins of tests/test_dist.py, copied) -------------------------------------
def _record(i, R=100, C=56):
    from pairnet_amd.dist import pack_triplets
    g = torch.Generator().manual_seed(1000 + i)
    labels = torch.randint(1, 134, (2 * R,), generator=g)
    rel = torch.rand(R, C + 1, generator=g)
    sub = torch.randint(0, 100, (R,), generator=g)
    obj = torch.randint(0, 100, (R,), generator=g)
    return pack_triplets(labels, rel, sub, obj)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _HostHead:
    num_rel_query, num_relations, device = 100, 56, None


class _HostDetector:
    def __init__(self, lag=3):
        self.bbox_head, self.lag, self.released = _HostHead(), lag, 0

    @staticmethod
    def detect(img):
        from pairnet_amd.dist import unpack_triplets
        i = int(img.flatten()[0])
        d = unpack_triplets(_record(i), 100, 56)
        res = (None, d["labels"], None, None, None, None, None, d["rel_dists"])
        return res, d["sub_pos"], d["obj_pos"]

    def stream_triplets(self, batches, rescale=False, depth=4):
        from pairnet_amd.dist import TripletBatch
        queue = []

        def rel(stream):
            self.released += 1
        for img, metas in batches:
            got = [self.detect(img[b]) for b in range(img.shape[0])]
            queue.append(TripletBatch([g[0] for g in got], [g[1] for g in got],
                                      [g[2] for g in got], stream=None, release=rel))
            if len(queue) > self.lag:
                yield queue.pop(0)
        while queue:
            yield queue.pop(0)


class _ListEvaluator:
    def __call__(self, res, gt_rels, gt_labels, gt_masks):
        n = len(gt_rels)
        base = int(res[1][0])
        p2g = [[(base + r) % n] if n and r % 3 == 0 else [] for r in range(100)]
        rec = {k: len({g for l in p2g[:k] for g in l}) / float(n) for k in (20, 50, 100)} if n else None
        return dict(pred_to_gt=p2g, phrdet_pred_to_gt=p2g, sgdet_recall=rec, phrdet_recall=rec)


def _streaming_list_evaluator():
    from pairnet_amd.evaluation import StreamingEvaluator

    class _StreamingListEvaluator(StreamingEvaluator):
        """`add` through `add_host` from `_ListEvaluator`'s lists: the loop only needs `add`,
        `state`, `merge` and `summary`."""

        def add(self, res, gt_rels, gt_labels, gt_masks, index=None, iou=True):
            self.add_host(index, _ListEvaluator()(res, gt_rels, gt_labels, gt_masks), gt_rels)
    return _StreamingListEvaluator(56)


def _host_dataset(n):
    return [(torch.full((1, 3, 2, 2), float(i)), [dict(img_shape=(2, 2, 3), scale_factor=[1.0] * 4)])
            for i in range(n)]


def _host_annotations(n):
    out = []
    for i in range(n):
        g = 0 if i == 1 else 2 + i % 3       # (image 1 has no ground-truth relations: skipped)
        rels = np.array([[j % 2, (j + 1) % 2, 1 + (i + j) % 56] for j in range(g)]).reshape(-1, 3)
        out.append(dict(gt_rels=rels, gt_labels=np.array([3, 7]), gt_masks=None))
    return out


def _existing_path_metrics(n):
    from pairnet_amd.dist import multi_gpu_test
    from pairnet_amd.evaluation import SceneGraphMetrics
    return multi_gpu_test(_HostDetector(), _host_dataset(n), annotations=_host_annotations(n),
                          evaluator=_ListEvaluator(), metrics=SceneGraphMetrics(56), depth=2)


def test_loop_takes_the_streaming_path_in_one_process():
    from pairnet_amd.dist import multi_gpu_test
    n = 5
    one = _existing_path_metrics(n)
    det, ev = _HostDetector(), _streaming_list_evaluator()
    out = multi_gpu_test(det, _host_dataset(n), annotations=_host_annotations(n), evaluator=ev,
                         depth=2)
    assert out["metrics"] == one["metrics"] and out["metrics"]["skipped"] == 1
    assert torch.equal(out["records"], one["records"]) and det.released == n
    assert sorted(ev.records()) == [0, 2, 3, 4]
    # `metrics=` is not needed on this path: ignored, with a warning
    from pairnet_amd.evaluation import SceneGraphMetrics
    unused = SceneGraphMetrics(56)
    with pytest.warns(UserWarning, match="ignored"):
        out2 = multi_gpu_test(_HostDetector(), _host_dataset(n), annotations=_host_annotations(n),
                              evaluator=_streaming_list_evaluator(), metrics=unused, depth=2)
    assert out2["metrics"] == one["metrics"] and unused.images == 0


def _loop_worker(rank, world, port, n_images, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pairnet_amd.dist import multi_gpu_test
    out = multi_gpu_test(_HostDetector(), _host_dataset(n_images),
                         annotations=_host_annotations(n_images),
                         evaluator=_streaming_list_evaluator(), depth=2)
    q.put((rank, out["records"].numpy(), out.get("metrics")))
    dist.barrier()
    dist.destroy_process_group()


def test_loop_streaming_path_world2_equals_world1_gloo():
    n = 5                                     # uneven split: rank 0 gets 3 images, rank 1 gets 2
    one = _existing_path_metrics(n)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world, port = 2, _free_port()
    procs = [ctx.Process(target=_loop_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = {r: rest for r, *rest in (q.get(timeout=120) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        assert torch.equal(torch.from_numpy(outs[r][0]), one["records"])
    assert outs[1][1] is None and outs[0][1] == one["metrics"]


# ---- refusals ------------------------------------------------------------------------------
def test_predicate_ids_outside_the_table_are_refused_on_the_host(images):
    from pairnet_amd.evaluation import StreamingEvaluator
    ev, gt_rels, _ = images[0]
    result = (None, torch.zeros(200, dtype=torch.int64), None, torch.zeros(200, 4, 4, dtype=torch.bool),
              None, None, None, torch.zeros(100, NUM_REL))
    boxes = (torch.zeros(200, 5), torch.zeros(200, dtype=torch.int64), None, None, None,
             torch.zeros(100, NUM_REL))
    for bad in (0, NUM_REL):
        rels = np.array(gt_rels)
        rels[1, 2] = bad
        se = StreamingEvaluator(56)
        with pytest.raises(ValueError, match="predicate"):   # before anything is enqueued
            se.add(result, rels, np.arange(1, 8), np.zeros((7, 4, 4), bool))
        with pytest.raises(ValueError, match="predicate"):
            se.add_boxes(boxes, rels, np.arange(1, 8), np.zeros((7, 4), np.float32))
        with pytest.raises(ValueError, match="predicate"):
            se.add_host(0, ev, rels)
        assert se.summary()["images"] == 0
    with pytest.raises(ValueError):
        StreamingEvaluator(56, ks=tuple(range(1, 10)))       # nk > 8
    with pytest.raises(ValueError):
        StreamingEvaluator(256)                              # num_rel > 256


def test_bad_arguments_are_refused_without_launching(built_lib):
    from pairnet_amd import hip
    lib = hip.lib()
    p = 16                                                   # (never dereferenced: refused first)
    ok = dict(ms=p, mp=p, R=100, G=9, gp=p, ks=p, nk=3, nr=57, hits=p, counts=p)

    def record(**kw):
        a = dict(ok, **kw)
        return lib.pn_eval_record(a["ms"], a["mp"], a["R"], a["G"], a["gp"], a["ks"], a["nk"],
                                  a["nr"], a["hits"], a["counts"], None)
    for k in ("ms", "mp", "gp", "ks", "hits", "counts"):
        assert record(**{k: None}) == -1, k
    for kw in (dict(nk=9), dict(nk=0), dict(nr=257), dict(nr=1), dict(R=0), dict(G=0),
               dict(R=-1), dict(G=-1)):
        assert record(**kw) == -1, kw
    ok = dict(inter=p, ap=p, ag=p, P=200, nobj=7, pl=p, gl=p, gs=p, go=p, G=9, valid=p, best=p)

    def iou(**kw):
        a = dict(ok, **kw)
        return lib.pn_eval_iou_best(a["inter"], a["ap"], a["ag"], a["P"], a["nobj"], a["pl"],
                                    a["gl"], a["gs"], a["go"], a["G"], a["valid"], a["best"], None)
    for k in ("inter", "ap", "ag", "pl", "gl", "gs", "go", "valid", "best"):
        assert iou(**{k: None}) == -1, k
    for kw in (dict(P=0), dict(nobj=0), dict(G=0), dict(G=-3)):
        assert iou(**kw) == -1, kw


# ---- declarations and compile ----------------------------------------------------------------
def test_header_and_binding_declare_the_new_entries():
    import pairnet_amd
    from pairnet_amd import build as B
    from pairnet_amd import hip
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    for name in ("pn_eval_record", "pn_eval_iou_best"):
        assert name in declared and name in hip._SIGS and name in hip.EXPORTS, name
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION
    assert callable(hip.eval_record) and callable(hip.eval_iou_best) and "evaluate" in B.SOURCES
    for cite in ("sgg_metrics.py:95-99", ":741-766", "sgg_metrics.py:1087-1131"):
        assert cite in header, cite
    assert pairnet_amd.StreamingEvaluator is pairnet_amd.evaluation.StreamingEvaluator
    assert "StreamingEvaluator" in pairnet_amd.api.__all__


def test_evaluate_kernels_compile_for_gfx950_without_scratch(tmp_path):
    from pairnet_amd import build as B
    out = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(B.CSRC, "evaluate.hip"), "-o", str(tmp_path / "evaluate.o")],
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
    kernels = {k: v for k, v in res.items() if "k_eval_record" in k or "k_eval_iou_best" in k}
    assert len(kernels) == 2, sorted(res)
    for k, use in kernels.items():
        print(k, use)
        assert use["ScratchSize [bytes/lane]"] == 0, k
        # (8 + 1) x 256 int histograms in the record kernel, none in the IoU kernel
        assert use["LDS Size [bytes/block]"] <= 9 * 256 * 4, k
