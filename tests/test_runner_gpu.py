"""GPU: pair-net_amd/runner.py and the trainer state behind it (`FlatTrainer.state_dict` /
`load_state_dict`), at the existing trainer tests' shapes: 96 x 128 images, B = 2, the ground truth
of tests/test_tri_train_gpu.py (3 and 5 objects); 128 x 160 for the box detector, the smallest it
accepts (tests/test_bbox_train_gpu.py).

  * resume is bitwise, per trainer: 4 steps straight against 2 steps, `save_checkpoint`, a fresh
    detector and trainer through `resume`, 2 steps;
  * the checkpoint file: `weights_only=True`, three keys, `load_checkpoint` round trip, no
    temporary file left;
  * `state_dict()["optimizer"]` loads into a real `torch.optim.AdamW`, and one further step of
    both agrees to the bound of tests/test_train_gpu.py::test_adamw_and_clip_kernels_equal_torch
    (2e-6 on the parameters);
  * the two log kernels against the fp32 left-to-right host computation, bit for bit;
  * no host wait in the runner's loop; the runner end to end, with a resumed second runner.

One run per trainer case is shared by the tests that read it (`_case_run`; never written)."""
import ctypes
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBJECTS = [3, 5]
ADAMW_PARAM_BOUND = 2e-6      # tests/test_train_gpu.py::test_adamw_and_clip_kernels_equal_torch
_RUNS = {}


# ------------------------------------------------------------------------------ the four cases
def _seeded(head, seed):
    from oracle import seeded
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in head.state_dict().items())
    head.load_state_dict(seeded.seeded_state_dict(shapes, seed))


def _mask_batch(H, W, seed=8):
    """Two images, 3 and 5 objects, the relations of tests/test_tri_train_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(2, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4, batch_input_shape=(H, W))] * 2
    gt_labels = [torch.randint(0, 133, (n,), generator=g) for n in OBJECTS]
    gt_masks = [(torch.rand(n, H, W, generator=g) > 0.6).numpy() for n in OBJECTS]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 0, 17], [1, 2, 55]]),
               torch.tensor([[0, 4, 2], [3, 1, 30], [4, 2, 9], [1, 0, 41]])]
    return dict(img=img, img_metas=metas, gt_rels=gt_rels, gt_bboxes=None, gt_labels=gt_labels,
                gt_masks=gt_masks)


def _box_batch(H, W):
    import bbox_loss_ref as R
    g = torch.Generator().manual_seed(7)
    img = torch.randn(2, 3, H, W, generator=g).to(DEV)
    metas = [dict(batch_input_shape=(H, W), img_shape=(H, W, 3), scale_factor=[1.0] * 4)] * 2
    case = R.make_case(seed=11, G=(4, 6), T=(3, 7), num_classes=150, num_relations=50,
                       batch_shape=(H, W), planted=False)
    return dict(img=img, img_metas=metas, gt_rels=case["gt_rels"], gt_bboxes=case["gt_bboxes"],
                gt_labels=case["gt_labels"])


def _case(name):
    """-> (config of the detector, seeding of a fresh one, trainer keywords, those `resume` must
    be given again, the batch)."""
    import pairnet_amd as P
    if name == "tail":
        return (P.pairnet_r50(), lambda d: d.bbox_head.init_weights(seed=4),
                dict(dropout=True, device_targets=True, deterministic=True), dict(dropout=True),
                _mask_batch(96, 128))
    if name == "baseline":
        return (P.baseline_r50(), lambda d: _seeded(d.bbox_head, 1234), dict(deterministic=True),
                {}, _mask_batch(96, 128))
    if name == "psgtr2":
        return (P.psgtr2_r50(), lambda d: _seeded(d.bbox_head, 1234), dict(deterministic=True),
                {}, _mask_batch(96, 128))
    assert name == "bbox"
    return (P.cross_r101_vg().model, lambda d: _seeded(d.bbox_head, 3), dict(device_targets=True),
            {}, _box_batch(128, 160))


def _step(det, tr, b):
    from pairnet_amd.runner import ENTRIES
    entry = ENTRIES[type(tr).__name__][0]
    args = (b["img"], b["img_metas"], b["gt_rels"], b.get("gt_bboxes"), b["gt_labels"])
    if entry != "box_train_step":
        args += (b["gt_masks"],)
    out = getattr(det, entry)(*args)
    return OrderedDict((k, v.clone()) for k, v in out.items())


def _snapshot(tr):
    torch.cuda.synchronize()
    return dict(p=tr.flat_p.clone(), m=tr.flat_m.clone(), v=tr.flat_v.clone(), steps=tr.steps,
                loss={k: v.clone() for k, v in tr._loss_buffers().items()})


def _case_run(name, tmp_root):
    """The straight run (4 steps) and the interrupted one (2 steps, checkpoint, `resume`, 2
    steps) of one trainer case, with what the tests read from them."""
    if name in _RUNS:
        return _RUNS[name]
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import pairnet_amd as P
    from pairnet_amd.runner import ENTRIES
    cfg, seed_weights, kw, again, batch = _case(name)

    def fresh(seed=True):
        det = P.build_detector(dict(cfg))
        if seed:
            seed_weights(det)
        return det.to(DEV)

    def trainer_of(det):
        return getattr(det, ENTRIES[P.runner.HEAD_TRAINER[type(det.bbox_head).__name__]][2])(**kw)

    # ---- straight: 4 steps; the state after 2, and the third step's gradient, on the way ----
    det_a = fresh()
    tr_a = trainer_of(det_a)
    torch.cuda.manual_seed(1)
    outs_a = [_step(det_a, tr_a, batch) for _ in range(2)]
    torch.cuda.synchronize()
    state2 = tr_a.state_dict()
    params2 = OrderedDict((n, v.cpu().clone()) for n, v in tr_a.params.items())
    grads = []
    plain = tr_a.apply_gradients

    def capture(*a, **k):
        grads.append(tr_a.flat_grad.clone())
        return plain(*a, **k)
    tr_a.apply_gradients = capture
    outs_a.append(_step(det_a, tr_a, batch))
    del tr_a.apply_gradients
    params3 = OrderedDict((n, v.cpu().clone()) for n, v in tr_a.params.items())
    outs_a.append(_step(det_a, tr_a, batch))
    end_a = _snapshot(tr_a)
    # ---- interrupted ----
    det_b = fresh()
    tr_b = trainer_of(det_b)
    torch.cuda.manual_seed(1)
    outs_b = [_step(det_b, tr_b, batch) for _ in range(2)]
    work = os.path.join(tmp_root, name)
    os.makedirs(work, exist_ok=True)
    path = os.path.join(work, "epoch_1.pth")
    P.save_checkpoint(det_b, tr_b, path, meta=dict(epoch=1, iter=2, seed=10086))
    saved_sd = {k: v.clone() for k, v in det_b.state_dict().items()}
    left = sorted(os.listdir(work))
    torch.cuda.manual_seed(999)                  # (the restored generator has to matter)
    det_c, tr_c, meta = P.resume(lambda: fresh(seed=False), path, **again)
    outs_c = [_step(det_c, tr_c, batch) for _ in range(2)]
    end_c = _snapshot(tr_c)
    _RUNS[name] = dict(det_a=det_a, tr_a=tr_a, outs_a=outs_a, end_a=end_a, outs_b=outs_b,
                       outs_c=outs_c, end_c=end_c, tr_c=tr_c, meta=meta, path=path, left=left,
                       saved_sd=saved_sd, state2=state2, params2=params2, params3=params3,
                       grad3=grads[0], batch=batch, fresh=fresh, kw=kw)
    return _RUNS[name]


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("runner"))


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------ resume
@pytest.mark.parametrize("name", ["tail", "baseline", "bbox", "psgtr2"])
def test_resume_is_bitwise(name, tmp_root):
    r = _case_run(name, tmp_root)
    a, c = r["end_a"], r["end_c"]
    assert a["steps"] == c["steps"] == 4 and type(r["tr_c"]) is type(r["tr_a"])
    for k in ("p", "m", "v"):
        assert torch.equal(_bits(a[k]), _bits(c[k])), k
    assert float(a["m"].abs().max()) > 0 and float(a["v"].abs().max()) > 0
    for i in (0, 1):                              # steps 1-2 agree (same start), steps 3-4 resumed
        assert list(r["outs_a"][i]) == list(r["outs_b"][i])
        assert list(r["outs_a"][2 + i]) == list(r["outs_c"][i])
        for k, v in r["outs_a"][2 + i].items():
            assert torch.equal(_bits(v), _bits(r["outs_c"][i][k])), (i, k)
            assert torch.equal(_bits(r["outs_a"][i][k]), _bits(r["outs_b"][i][k])), (i, k)
        assert int(r["outs_c"][i]["assign_status"]) == 0
    assert set(a["loss"]) == set(c["loss"])
    for k, v in a["loss"].items():
        assert torch.equal(_bits(v), _bits(c["loss"][k])), k
    if name in ("tail", "bbox"):                  # SeesawLoss's counts: 4 steps of 7 (10) relations
        cum = a["loss"]["rel_cls_loss.cum_samples"]
        assert float(cum.sum()) == 4 * sum(len(x) for x in r["batch"]["gt_rels"])
    else:
        assert not a["loss"]
    # the moments moved between the checkpoint and the end: the resumed steps did train
    assert r["meta"]["trainer"]["steps"] == 2 and r["meta"]["epoch"] == 1 and r["meta"]["iter"] == 2
    # a state of another class, or other flags, is refused by name
    sd = r["tr_c"].state_dict()
    with pytest.raises(ValueError, match="NoSuchTrainer"):
        r["tr_c"].load_state_dict(dict(sd, trainer=dict(sd["trainer"], **{"class": "NoSuchTrainer"})))


@pytest.mark.parametrize("name", ["tail", "bbox"])
def test_checkpoint_file(name, tmp_root):
    import pairnet_amd as P
    r = _case_run(name, tmp_root)
    assert r["left"] == ["epoch_1.pth"]                               # no temporary file
    ckpt = torch.load(r["path"], map_location="cpu", weights_only=True)
    assert set(ckpt) == {"meta", "state_dict", "optimizer"}
    meta = ckpt["meta"]
    assert meta["version"] == P.runner.CHECKPOINT_VERSION and meta["seed"] == 10086
    block = meta["trainer"]
    assert block["class"] == type(r["tr_a"]).__name__ and block["steps"] == 2
    assert block["device_targets"] is True
    gens = block["generators"]
    assert all(v.dtype == torch.uint8 for v in gens.values())
    assert ("device_default" in gens) == (name == "tail") and ("drop_path" in gens) == (name == "tail")
    loss_key = "bbox_head.rel_cls_loss.cum_samples"
    assert loss_key in ckpt["state_dict"]
    assert torch.equal(ckpt["state_dict"][loss_key], block["loss"]["rel_cls_loss.cum_samples"])
    opt = ckpt["optimizer"]
    assert opt["param_names"] == list(r["tr_a"].names) and len(opt["param_groups"]) == len(opt["state"])
    assert [g["params"] for g in opt["param_groups"][:3]] == [[0], [1], [2]]
    frozen = [n for n in r["tr_a"].layout if n not in r["tr_a"].params]
    assert (len(frozen) > 0) == (name == "tail") and not set(frozen) & set(opt["param_names"])
    # weights only: the existing load_checkpoint into a fresh detector
    det = r["fresh"](seed=False)
    with pytest.warns(UserWarning, match="unexpected"):              # (the loss buffer's key)
        P.load_checkpoint(det, r["path"])
    got = det.state_dict()
    assert set(got) == set(r["saved_sd"]) == set(ckpt["state_dict"]) - {loss_key}
    for k, v in r["saved_sd"].items():
        assert torch.equal(_bits(got[k].cpu()), _bits(v.cpu())), k
    moved = [k for k, v in ckpt["state_dict"].items() if k.startswith("bbox_head.relation_decoder")]
    assert moved


def test_optimizer_state_loads_into_torch_adamw(tmp_root):
    """The AdamW block after two steps, in a real torch.optim.AdamW over host copies of the
    parameters (one group each, `param_names` order); then the trainer's own third-step gradient
    on both sides (the host's clipped by `clip_grad_norm_`), parameter by parameter."""
    r = _case_run("tail", tmp_root)
    tr, opt_sd = r["tr_a"], r["state2"]["optimizer"]
    names = opt_sd["param_names"]
    assert names == list(tr.names) and r["state2"]["trainer"]["steps"] == 2
    host = [r["params2"][n].double().requires_grad_() for n in names]
    opt = torch.optim.AdamW([dict(params=[p]) for p in host], lr=1.0)
    opt.load_state_dict(opt_sd)                                       # must not raise
    g0 = opt.param_groups[names.index("rel_cls_embed.weight")]
    assert g0["lr"] == pytest.approx(tr.lr) and g0["betas"] == (0.9, 0.999) and not g0["amsgrad"]
    bb = opt.param_groups[names.index("backbone.layer3.2.conv2.weight")]
    assert bb["lr"] == pytest.approx(0.1 * tr.lr) and bb["initial_lr"] == pytest.approx(0.1 * tr.lr)
    assert float(opt.state[host[0]]["step"]) == 2.0
    grad = r["grad3"].cpu()
    for p, n in zip(host, names):
        o, shape, k = tr.layout[n]
        p.grad = grad[o:o + k].view(shape).double()
    norm = torch.nn.utils.clip_grad_norm_(host, tr.max_norm)
    assert float(norm) > 0
    opt.step()
    worst = 0.0
    for p, n in zip(host, names):
        err = float((r["params3"][n].double() - p.detach()).abs().max())
        worst = max(worst, err)
        assert err < ADAMW_PARAM_BOUND, (n, err)
        assert not torch.equal(r["params3"][n], r["params2"][n]), n   # (it did move)
    print("third step against torch.optim.AdamW from the loaded state: worst |difference| %.2e" % worst)


# ------------------------------------------------------------------------------ the log kernels
def _host_window(rows, T, mask):
    """fp32, left to right: the per-row loss sums, then the means of the T + 1 columns."""
    f = np.float32
    table = []
    for vals in rows:
        loss = f(0)
        for i in range(T):
            if (mask >> i) & 1:
                loss = f(loss + vals[i])
        table.append(list(vals) + [loss])
    means = []
    for c in range(T + 1):
        s = table[0][c]
        for row in table[1:]:
            s = f(s + row[c])
        means.append(f(s / f(len(table))))
    return np.array(means, f)


@pytest.mark.parametrize("T,n,interval", [(1, 4, 4), (5, 7, 7), (32, 50, 50), (5, 3, 8), (32, 1, 2)])
def test_log_kernels_equal_the_host_computation(T, n, interval):
    """Window means bit for bit, at T = 1, 5, 32; (5, 3, 8) and (32, 1, 2) are windows cut short
    (n < interval rows); the status words OR-ed, the skipped rows counted."""
    from pairnet_amd import hip
    rng = np.random.default_rng(100 * T + n)
    vals = (rng.standard_normal((n, T)) * 10.0 ** rng.integers(-3, 3, (n, T))).astype(np.float32)
    mask = int(rng.integers(1, 2 ** T)) if T < 32 else 0xBFFFFFFF
    st0 = rng.integers(0, 2, n) * rng.integers(1, 9, n)
    st1 = (rng.integers(0, 4, n) == 0) * 16
    ring = torch.full((interval, T + 3), 7.0, device=DEV)
    rec = torch.zeros(T + 4, device=DEV)
    for r in range(n):
        # separate 0-dim tensors, as a step's dict holds them
        scalars = [torch.tensor(float(v), device=DEV) for v in vals[r]]
        s0 = torch.tensor([int(st0[r])], dtype=torch.int32, device=DEV)
        s1 = torch.tensor([int(st1[r])], dtype=torch.int32, device=DEV)
        hip.train_log_row(scalars, mask, [s0, s1] if r % 2 else [s0, None], ring, r)
        if r % 2 == 0:
            st1[r] = 0
    hip.train_log_window(ring, n, T, rec)
    torch.cuda.synchronize()
    got = rec.cpu()
    want = _host_window(vals, T, mask)
    assert np.array_equal(got[:T + 1].numpy().view(np.uint32), want.view(np.uint32))
    status = st0 | st1
    ints = got.view(torch.int32)[T + 1:].tolist()
    assert ints == [int((status != 0).sum()), int(np.bitwise_or.reduce(status)), n]
    ring_h = ring.cpu()
    assert np.array_equal(ring_h[:n, :T].numpy().view(np.uint32), vals.view(np.uint32))
    assert ring_h[:n, T + 1].view(torch.int32).tolist() == status.tolist()
    assert (ring_h[n:] == 7.0).all()                                  # rows past n: untouched


def test_log_kernels_refuse_bad_arguments():
    from pairnet_amd import hip
    lib = hip.lib()
    buf = torch.zeros(4096, device=DEV)
    at = lambda i: buf.data_ptr() + 4 * i
    ptrs = lambda n, null=None: (ctypes.c_void_p * n)(*[None if i == null else at(i)
                                                          for i in range(n)])
    ring, rec = ctypes.c_void_p(at(64)), ctypes.c_void_p(at(2048))
    good = [ptrs(32), 32, 0xffffffff, None, None, ring, 50, 35, 49, None]
    assert lib.pn_train_log_row_f32(*good) == 0
    for i, v in ((1, 33), (1, 0), (0, None), (5, None), (0, ptrs(32, null=31)), (0, ptrs(32, null=0)),
                 (7, 34), (8, 50), (8, -1), (6, 0)):
        args = list(good)                                             # T = 33, T = 0, NULL table /
        args[i] = v                                                   # ring / scalar, ld, row, rows
        assert lib.pn_train_log_row_f32(*args) == -1, (i, v)
    good = [ring, 50, 35, 50, 32, rec, None]
    assert lib.pn_train_log_window_f32(*good) == 0
    for i, v in ((0, None), (5, None), (4, 33), (4, 0), (2, 34), (3, 0), (3, 51)):
        args = list(good)
        args[i] = v
        assert lib.pn_train_log_window_f32(*args) == -1, (i, v)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        hip.train_log_row([buf[i] for i in range(33)], 1, [], buf[:70].view(2, 35), 0)


def test_train_log_with_a_skipped_step(tmp_root):
    """Three steps of the triplet trainer in one window, the second with a ground-truth relation
    out of range (as tests/test_tri_train_gpu.py::test_a_refused_assignment_moves_no_parameter
    plants it): `skipped == 1`, the OR of the status words is reported, that step's parameters do
    not move, and the means are the host's fp32 left-to-right ones of the values the steps
    returned (a refused step's terms may be NaN: then both sides are)."""
    import pairnet_amd as P
    r = _case_run("psgtr2", tmp_root)
    det, tr, b = r["det_a"], r["tr_a"], r["batch"]
    bad = dict(b, gt_rels=[b["gt_rels"][0].to(DEV),
                           torch.tensor([[0, 7, 2], [3, 1, 30]], device=DEV)])
    path = os.path.join(tmp_root, "skipped.log.json")
    log = P.TrainLog(DEV, interval=3, path=path)
    outs, moved = [], []
    for i, batch in enumerate((b, bad, b)):
        before = tr.flat_p.clone()
        out = _step(det, tr, batch)
        outs.append(out)
        moved.append(not torch.equal(_bits(before), _bits(tr.flat_p)))
        log.add(out, epoch=1, iter=i + 1, lr=tr.lr, time=0.5, data_time=0.25)
    assert log.count == 0 and len(log._pending) == 1                 # the window closed itself
    log.flush()
    assert moved == [True, False, True]
    status = [int(o["assign_status"]) for o in outs]
    assert status[0] == 0 and status[1] != 0 and status[2] == 0
    rec, = log.records
    assert rec["skipped"] == 1 and rec["status"] == status[1] and rec["n"] == 3
    names = [k for k in outs[0] if k != "assign_status"]
    T = len(names)
    assert names[-1] == "grad_norm" and T == 8
    mask = sum(1 << i for i, k in enumerate(names) if "loss" in k)
    want = _host_window([[np.float32(float(o[k])) for k in names] for o in outs], T, mask)
    got = np.array([rec[k] for k in names] + [rec["loss"]], np.float32)
    assert np.array_equal(got, want, equal_nan=True)
    line = json.loads(open(path).read().strip().splitlines()[-1], object_pairs_hook=OrderedDict)
    assert list(line) == ["mode", "epoch", "iter", "lr", "time", "data_time"] + names[:-1] + \
        ["loss", "grad_norm", "skipped", "status"]
    assert line["mode"] == "train" and line["iter"] == 3 and line["time"] == 0.5


# ------------------------------------------------------------------------------ the runner
def _ready_batches(det, b, k):
    """k ready batch dicts (the masks prepared once, on the device: nothing left to upload but the
    ground-truth tables the loss sends itself)."""
    from pairnet_amd import HalfSizeMasks
    H, W = b["img"].shape[2:]
    masks = [HalfSizeMasks(m, (H, W)) for m in det._prepare_gt_masks(b["img"], b["gt_masks"])]
    out = []
    for i in range(k):
        img = b["img"] + 0.01 * i
        out.append(dict(b, img=img, gt_masks=masks))
    return out


def test_no_host_wait_in_the_loop(tmp_root):
    import pairnet_amd as P
    # (the relation tail's scope, the one tests/test_device_targets_gpu.py holds to "no host wait":
    # the pixel-decoder tape of the wider scopes uploads a small pageable table per step, which
    # torch's detector flags)
    r = _case_run("tail", tmp_root)
    det = r["fresh"]()
    tr = det.trainer(train_decoder=False, train_pixel_decoder=False, device_targets=True)
    assert tr.device_targets and tr.backbone is None
    data = _ready_batches(det, r["batch"], 4)
    run = P.EpochRunner(det, tr, data, log_interval=3, max_epochs=1, shuffle=False,
                        work_dir=os.path.join(tmp_root, "nowait"), ckpt_interval=0)
    run.train_epoch(0)                            # warm-up: buffers, the log's ring, pinned records
    assert [x["n"] for x in run.log.records] == [3, 1]
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run.train_epoch(1, flush=False)           # 4 steps, a window boundary, the cut-short window
        run.log.poll()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    run.log.flush()
    assert [x["n"] for x in run.log.records] == [3, 1, 3, 1]
    assert [x["epoch"] for x in run.log.records] == [1, 1, 2, 2] and run.iter == 8
    assert all(np.isfinite(x["loss"]) and x["skipped"] == 0 for x in run.log.records)


def test_runner_end_to_end_and_resumed(tmp_root):
    import pairnet_amd as P
    r = _case_run("tail", tmp_root)
    cfg, seed_weights, kw, again, batch = _case("tail")
    work = os.path.join(tmp_root, "e2e")
    args = dict(max_epochs=3, lr_steps=(1, 2), lr_gamma=0.5, ckpt_interval=1, max_keep_ckpts=2,
                log_interval=2, seed=5)

    def detector(seed=True):
        det = r["fresh"](seed=seed)
        return det, _ready_batches(det, batch, 2)
    det, data = detector()
    torch.cuda.manual_seed(3)
    first = os.path.join(tmp_root, "e2e_epoch_1.pth")

    class KeepsTheFirst(P.EpochRunner):
        """epoch_1.pth is pruned by the end of the run: a copy of it, to resume from."""
        def save(self):
            name = super().save()
            if name == "epoch_1.pth":
                with open(os.path.join(work, name), "rb") as f, open(first, "wb") as g:
                    g.write(f.read())
            return name
    full = KeepsTheFirst(det, det.trainer(**kw), data, work_dir=work, **args)
    full.run()
    tr = full.trainer
    assert sorted(os.listdir(work)) == sorted(["epoch_2.pth", "epoch_3.pth", "latest.pth",
                                               os.path.basename(full.log_path)])
    assert os.readlink(os.path.join(work, "latest.pth")) == "epoch_3.pth"
    lines = [json.loads(x) for x in open(full.log_path).read().splitlines()]
    assert [(x["epoch"], x["iter"]) for x in lines] == [(1, 2), (2, 2), (3, 2)]
    base = tr.base_lr
    assert [x["lr"] for x in lines] == [P.train.step_lr(base, e, (1, 2), 0.5) for e in range(3)]
    assert [x["lr"] for x in lines] == [base, base * 0.5, base * 0.25] and tr.steps == 6
    assert [e for e, _ in full.handed] == [0, 0, 1, 1, 2, 2]
    for e in range(3):
        assert [i for ep, idx in full.handed if ep == e for i in idx] == P.epoch_order(2, e, 5)
    # ---- a second runner from epoch_1.pth, fresh detector, other weights until it loads ----
    det2, data2 = detector(seed=False)
    torch.cuda.manual_seed(77)
    second = P.EpochRunner(det2, None, data2, work_dir=os.path.join(tmp_root, "e2e_resumed"),
                           resume_from=first, trainer_kw=again, **args)
    second.run()
    tr2 = second.trainer
    assert tr2.steps == 6 and second.epoch == 3 and second.iter == 6
    assert second.handed == full.handed[2:]
    for k in ("flat_p", "flat_m", "flat_v"):
        assert torch.equal(_bits(getattr(tr, k)), _bits(getattr(tr2, k))), k
    assert tr2.base_lr == base and tr2.lr == base * 0.25
