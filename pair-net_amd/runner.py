"""Training for epochs, and resuming: what lies between "one iteration is correct" (the four
trainers on `FlatTrainer`) and "a model can be trained" -- the reference's tools/train.py:115-241
with mmcv's `EpochBasedRunner`, `StepLrUpdaterHook`, `CheckpointHook` and `TextLoggerHook` behind
the `runner` / `lr_config` / `checkpoint_config` / `log_config` / `auto_scale_lr` / `resume_from` /
`load_from` keys that configs/_base_/custom_runtime.py and configs/mask2former/pairnet.py:352-394
set.  mmcv is not a dependency: nothing here imports it.

    runner = EpochRunner.from_config(cfg, det, dataset, work_dir)       # or EpochRunner(det, ...)
    runner.run()

    save_checkpoint(det, trainer, "epoch_3.pth", meta=dict(epoch=3, iter=...))
    det, trainer, meta = resume(lambda: build_detector(cfg.model).to("cuda:0"), "epoch_3.pth")

* `save_checkpoint` / `resume`: mmcv's three keys {"meta", "state_dict", "optimizer"}; the
  optimizer block is `FlatTrainer.state_dict()`'s (torch.optim.AdamW's layout), the rest of the
  trainer's state travels in `meta["trainer"]`.  A resumed run continues bit for bit
  (tests/test_runner_gpu.py).
* `epoch_order`: `torch.utils.data.DistributedSampler`'s order.
* `TrainLog`: the per-iteration log on the device (csrc/train_log.hip) -- no `float()` per term
  and step; one JSON line per window once its record has arrived on the host.
* `EpochRunner`: the loop.

UNPINNED (restated from memory of mmcv, which does not import where this was written): the JSON
log's field order, `CheckpointHook`'s file names and pruning, `StepLrUpdaterHook` by epoch, one
optimizer param group per parameter under a `paramwise_cfg`.  One deliberate difference: mmcv's
logger hooks drop a window that the epoch's end cuts short (`ignore_last=True`); this one writes
it, averaged over the iterations it holds.
"""
import inspect
import json
import math
import os
import time
import warnings
from collections import OrderedDict

import numpy as np
import torch

from . import hip
from .detector import TRAIN_ENTRIES, load_checkpoint

__all__ = ["EpochRunner", "TrainLog", "save_checkpoint", "resume", "epoch_order",
           "auto_scaled_lr", "CHECKPOINT_VERSION"]

CHECKPOINT_VERSION = "pairnet_amd-ckpt-1"
DEFAULT_SEED = 10086        # tools/train.py:204 hard-codes it

# two views of the detector's table (detector.TRAIN_ENTRIES, one row per trainer):
# trainer class -> (the detector's step entry, where the detector keeps the trainer, its builder)
ENTRIES = {name: (row.step, row.slot, row.builder) for name, row in TRAIN_ENTRIES.items()}
HEAD_TRAINER = {row.head: name for name, row in TRAIN_ENTRIES.items()}


# ---------------------------------------------------------------------------- checkpoints
def save_checkpoint(det, trainer, filename, meta=None):
    """mmcv's `save_checkpoint` for a detector trained by a `FlatTrainer`: `trainer.write_back()`,
    then {"meta", "state_dict", "optimizer"} -- `state_dict` is `det.state_dict()` (the
    reference's key names) plus the loss's persistent buffers under the names the loss object's
    own `state_dict()` uses, prefixed `bbox_head.` (SeesawLoss's `rel_cls_loss.cum_samples`);
    `optimizer` is the trainer's AdamW block; `meta` carries `epoch`, `iter`, `seed`, the
    trainer's block and a version string.  Tensors and plain containers only: the file loads with
    `torch.load(..., weights_only=True)`.  Written under a temporary name and renamed, so a killed
    run leaves no half-written file."""
    trainer.write_back()
    tsd = trainer.state_dict()
    sd = OrderedDict(det.state_dict())
    for k, v in tsd["trainer"]["loss"].items():
        sd["bbox_head." + k] = v
    m = dict(meta or {})
    m.setdefault("epoch", 0)
    m.setdefault("iter", int(trainer.steps))
    m.setdefault("seed", None)
    m["trainer"] = tsd["trainer"]
    m["version"] = CHECKPOINT_VERSION
    filename = os.fspath(filename)
    tmp = "%s.tmp.%d" % (filename, os.getpid())
    try:
        torch.save({"meta": m, "state_dict": sd, "optimizer": tsd["optimizer"]}, tmp)
        os.replace(tmp, filename)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return filename


def _build_trainer(det, cls_name, trainer_kw):
    entry = ENTRIES.get(cls_name)
    if entry is None:
        raise ValueError("no training step for a %r (built: %s)" % (cls_name, sorted(ENTRIES)))
    return getattr(det, entry[2])(**trainer_kw)


def _restore(det, filename, trainer_kw):
    """Weights first (the existing `load_checkpoint`), then the trainer (its constructor copies
    the loaded parameters into `flat_p`), then the trainer's state."""
    with warnings.catch_warnings():
        # (the loss buffers beside the parameters are no key of `det.state_dict()`: told apart
        # below, every other difference is reported)
        warnings.simplefilter("ignore")
        ckpt = load_checkpoint(det, filename)
    meta = ckpt.get("meta") or {}
    if "trainer" not in meta or "optimizer" not in ckpt:
        raise ValueError("%s holds no training state (meta['trainer'] / 'optimizer'): it can be "
                         "loaded as weights (load_from), not resumed" % filename)
    block = meta["trainer"]
    own, keys = set(det.state_dict()), set(ckpt["state_dict"])
    keys = {k[len("module."):] if k.startswith("module.") else k for k in keys}
    unexpected = keys - own - {"bbox_head." + k for k in block.get("loss", {})}
    if own - keys or unexpected:
        warnings.warn("resume: %d missing key(s) (first: %s), %d unexpected (first: %s)"
                      % (len(own - keys), sorted(own - keys)[:2], len(unexpected),
                         sorted(unexpected)[:2]))
    kw = dict(trainer_kw)
    from . import api
    if block["class"] in ENTRIES:         # (any other class: `_build_trainer` refuses it by name)
        accepted = inspect.signature(getattr(api, block["class"]).__init__).parameters
        for key in ("deterministic", "device_targets", "seed"):
            if key in accepted and key in block:
                kw.setdefault(key, block[key])
    kw.setdefault("lr", block["base_lr"])
    trainer = _build_trainer(det, block["class"], kw)
    trainer.load_state_dict({"optimizer": ckpt["optimizer"], "trainer": block})
    return trainer, meta


def resume(det_builder, filename, **trainer_kw):
    """`resume_from`: `det_builder()` -> a fresh detector on its device; returns (det, trainer,
    meta) ready for the next step.  The trainer is the one of the checkpoint's class, built
    through the detector (`trainer()` / `full_trainer()` / `box_trainer()` / `triplet_trainer()`)
    with `trainer_kw`; `deterministic`, `device_targets` and `seed` default to the saved ones.
    What a trainer's constructor takes and its state does not hold (`dropout=`, `drop_path=`,
    `lr_mult=` ...) is the caller's to repeat.  (`load_from` -- weights only, epoch and iteration
    0 -- is `load_checkpoint`.)"""
    det = det_builder()
    trainer, meta = _restore(det, filename, trainer_kw)
    return det, trainer, meta


# ---------------------------------------------------------------------------- sampler, lr
def epoch_order(N, epoch, seed=0, rank=0, world=1, shuffle=True):
    """The indices `torch.utils.data.DistributedSampler(range(N), world, rank, shuffle, seed)`
    hands out after `set_epoch(epoch)` (drop_last=False): `randperm` under `manual_seed(seed +
    epoch)`, padded to a multiple of `world` by wrapping around, strided by rank.  mmdet's
    aspect-ratio `GroupSampler` / `DistributedGroupSampler` is NOT restated: batches here mix
    landscape and portrait images (`TrainPipeline.batch` pads to the largest)."""
    N, world, rank = int(N), int(world), int(rank)
    if N < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError("epoch_order: N >= 1, world >= 1, 0 <= rank < world")
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) + int(epoch))
        idx = torch.randperm(N, generator=g).tolist()
    else:
        idx = list(range(N))
    total = -(-N // world) * world
    pad = total - N
    if pad <= N:
        idx += idx[:pad]
    else:
        idx += (idx * math.ceil(pad / N))[:pad]
    return idx[rank:total:world]


def auto_scaled_lr(lr, auto_scale_lr, world, samples_per_gpu):
    """mmdet's `auto_scale_lr` (tools/train.py:129-141 hands the key to it): when enabled,
    lr x (world x samples_per_gpu) / base_batch_size."""
    a = auto_scale_lr or {}
    if not a.get("enable", False):
        return float(lr)
    if "base_batch_size" not in a:
        raise ValueError("auto_scale_lr.enable without auto_scale_lr.base_batch_size")
    return float(lr) * (int(world) * int(samples_per_gpu)) / float(a["base_batch_size"])


# ---------------------------------------------------------------------------- the log
class TrainLog:
    """The training log, kept on the device (csrc/train_log.hip).  `add(out)` is ONE launch: the
    step's scalars (every entry of the step's dict but `assign_status`: the loss terms, then
    `grad_norm`), their `loss` sum, the status word and the skipped flag go into row `iter %
    interval` of a device ring.  `close_window()` is a second launch (means in row order, skipped
    count, OR of the status words) and an asynchronous copy of that record into pinned host
    memory on a side stream, behind an event.  The host formats a window only once its event has
    completed: `poll()` never waits, `flush()` does.  `records`: the windows emitted so far."""
    SLOTS = 4       # windows in flight before `close_window` has to wait for the oldest

    def __init__(self, device, interval=50, path=None):
        self.device = torch.device(device)
        self.interval = int(interval)
        if self.interval < 1:
            raise ValueError("log interval >= 1")
        self.path, self.records = path, []
        self.names, self.count, self._pending, self._free = None, 0, [], list(range(self.SLOTS))
        self._info = None

    def _setup(self, names):
        T = len(names)
        if not 1 <= T <= hip.LOG_MAX_TERMS:
            raise ValueError("%d scalars per step; the log launch carries 1 .. %d"
                             % (T, hip.LOG_MAX_TERMS))
        self.names, self.T = list(names), T
        self.mask = sum(1 << i for i, n in enumerate(names) if "loss" in n)
        dev = self.device
        self.ring = torch.zeros(self.interval, T + 3, device=dev, dtype=torch.float32)
        self._dev = torch.zeros(self.SLOTS, T + 4, device=dev, dtype=torch.float32)
        self._host = torch.zeros(self.SLOTS, T + 4, dtype=torch.float32).pin_memory()
        self._side = torch.cuda.Stream(device=dev)
        self._events = [torch.cuda.Event() for _ in range(self.SLOTS)]

    @hip.on_device
    def add(self, out, **info):
        """One step's dict -> one ring row.  `info` (epoch, iter, lr, time, data_time ...): host
        values kept for the window's line; `time` / `data_time` are averaged over the window."""
        names = [k for k in out if k != "assign_status"]
        if self.names is None:
            self._setup(names)
        elif names != self.names:
            raise ValueError("the step's terms changed: %s, then %s" % (self.names, names))
        hip.train_log_row([out[k] for k in names], self.mask, [out.get("assign_status")],
                          self.ring, self.count)
        self.count += 1
        acc = self._info = self._info or dict(time=0.0, data_time=0.0)
        acc["time"] += float(info.pop("time", 0.0))
        acc["data_time"] += float(info.pop("data_time", 0.0))
        acc.update(info)
        if self.count == self.interval:
            self.close_window()

    @hip.on_device
    def close_window(self):
        """The window's record (no-op on an empty window); polls the earlier ones first."""
        self.poll()
        n = self.count
        if n == 0:
            return
        if not self._free:                    # SLOTS windows in flight: wait for the oldest
            self._pending[0][1].synchronize()
            self.poll()
        slot = self._free.pop(0)
        hip.train_log_window(self.ring, n, self.T, self._dev[slot])
        cur = torch.cuda.current_stream(self.device)
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            self._host[slot].copy_(self._dev[slot], non_blocking=True)
            self._events[slot].record(self._side)
        info = dict(self._info, n=n)
        info["time"], info["data_time"] = info["time"] / n, info["data_time"] / n
        self._pending.append((slot, self._events[slot], info))
        self.count, self._info = 0, None

    def poll(self):
        """Emit the windows whose record has arrived, oldest first; never waits."""
        while self._pending and self._pending[0][1].query():
            self._emit(*self._pending.pop(0))

    def flush(self):
        """Close the open window and wait for every record (the epoch's end)."""
        self.close_window()
        while self._pending:
            self._pending[0][1].synchronize()
            self._emit(*self._pending.pop(0))

    def _emit(self, slot, event, info):
        rec = self._host[slot]
        vals = rec[:self.T + 1].numpy().copy()
        skipped, status, n = (int(v) for v in rec.view(torch.int32)[self.T + 1:self.T + 4])
        self._free.append(slot)
        assert n == info["n"], (n, info)
        line = OrderedDict(mode="train")
        for k in ("epoch", "iter", "lr", "time", "data_time"):
            if k in info:
                line[k] = info[k]
        terms = OrderedDict((k, float(v)) for k, v in zip(self.names, vals[:self.T]))
        grad_norm = terms.pop("grad_norm", None)
        line.update(terms)
        line["loss"] = float(vals[self.T])
        if grad_norm is not None:
            line["grad_norm"] = grad_norm
        line["skipped"] = skipped
        if skipped:
            line["status"] = status
        self.records.append(dict(line, n=n, status=status))
        if self.path is not None:
            with open(self.path, "a") as f:
                f.write(json.dumps(line) + "\n")


# ---------------------------------------------------------------------------- the runner
def _rng_state(rng):
    kind, keys, pos, has_gauss, cached = rng.get_state()
    return dict(kind=kind, keys=torch.from_numpy(keys.astype(np.int64)), pos=int(pos),
                has_gauss=int(has_gauss), cached=float(cached))


def _set_rng_state(rng, s):
    rng.set_state((s["kind"], s["keys"].numpy().astype(np.uint32), int(s["pos"]),
                   int(s["has_gauss"]), float(s["cached"])))


class EpochRunner:
    """mmcv's `EpochBasedRunner` with the hooks the reference's configs register, for a detector
    of this package and its `FlatTrainer`:

    per epoch  `trainer.set_epoch(epoch, lr_steps, lr_gamma)`; the epoch's order from
               `epoch_order` (this rank's share); per iteration the batch -- `dataset[i]` is
               either a ready batch dict (img, img_metas, gt_rels, gt_bboxes, gt_labels, gt_masks:
               one index per iteration) or a raw sample for `pipeline.batch` (`samples_per_gpu`
               indices per iteration, the last batch may be short; the pipeline's draws come from
               a generator the runner owns and checkpoints; a batch whose crop keeps no relation
               draws other images, as mmdet's dataset does) -- then the detector's own step entry
               for the trainer's class (`train_step`, `full_train_step`, `box_train_step`,
               `triplet_train_step`) and ONE log launch (`TrainLog`);
    epoch end  the log is flushed (the loop's only wait); after every `ckpt_interval` epochs
               rank 0 writes `epoch_{n}.pth`, prunes all but the newest `max_keep_ckpts` (<= 0:
               keeps all) and points the relative symlink `latest.pth` at it.

    `trainer=None`: built through the detector when the run starts (after `load_from` /
    `resume_from` have loaded their weights) with `trainer_kw`.  `run(start=meta)` continues from
    a checkpoint's `meta`; `resume_from=` does both.  Resuming happens at epoch boundaries, where
    the checkpoints are written.  `group`: passed to the trainer (data-parallel gradient
    averaging; `TailTrainer` only) and read for rank / world size."""

    def __init__(self, det, trainer, dataset, *, pipeline=None, samples_per_gpu=2, max_epochs=15,
                 lr_steps=(5, 10), lr_gamma=0.5, ckpt_interval=1, max_keep_ckpts=1,
                 log_interval=50, work_dir, seed=DEFAULT_SEED, shuffle=True, group=None,
                 resume_from=None, load_from=None, trainer_kw=None):
        self.det, self.trainer, self.dataset, self.pipeline = det, trainer, dataset, pipeline
        self.samples_per_gpu, self.max_epochs = int(samples_per_gpu), int(max_epochs)
        self.lr_steps = tuple(int(s) for s in ([lr_steps] if isinstance(lr_steps, int) else lr_steps))
        self.lr_gamma = float(lr_gamma)
        self.ckpt_interval, self.max_keep_ckpts = int(ckpt_interval), int(max_keep_ckpts)
        self.log_interval = int(log_interval)
        self.work_dir = os.fspath(work_dir)
        self.seed, self.shuffle, self.group = int(seed), bool(shuffle), group
        self.resume_from, self.load_from = resume_from, load_from
        self.trainer_kw = dict(trainer_kw or {})
        if trainer is not None and (resume_from or load_from):
            raise ValueError("resume_from / load_from load weights into the detector: pass "
                             "trainer=None (it is built after them, from `trainer_kw`)")
        self.rank, self.world = 0, 1
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            self.rank, self.world = int(dist.get_rank(group)), int(dist.get_world_size(group))
        self.rng = np.random.RandomState(self.seed + self.rank)     # the pipeline's draws
        self.epoch, self.iter = 0, 0
        self.handed = []          # (epoch, [dataset indices]) of every iteration of this run
        self.log = None
        if trainer is not None:
            self._adopt(trainer)

    # ------------------------------------------------------------------ configuration
    @classmethod
    def from_config(cls, cfg, det, dataset, work_dir, **kw):
        """The reference's file-level config (`load_config(path)`, or the restated
        `pairnet_r50(schedule=True)`): `runner`, `lr_config`, `checkpoint_config`,
        `log_config`, `data.samples_per_gpu`, `optimizer.lr` with `auto_scale_lr`, `resume_from`,
        `load_from`.  What the runner does not implement is refused with `NotImplementedError`
        naming the key.  Keywords override (pipeline=, seed=, trainer_kw=, group= ...)."""
        get = lambda d, k, default=None: (d.get(k, default) if d is not None else default)
        runner = cfg.get("runner") or dict(type="EpochBasedRunner", max_epochs=15)
        if runner.get("type", "EpochBasedRunner") != "EpochBasedRunner":
            raise NotImplementedError("runner.type=%r (built: EpochBasedRunner; IterBasedRunner "
                                      "is not)" % (runner.get("type"),))
        lrc = cfg.get("lr_config") or dict(policy="step", step=[])
        if lrc.get("policy", "step") != "step":
            raise NotImplementedError("lr_config.policy=%r (built: 'step')" % (lrc.get("policy"),))
        if lrc.get("warmup") is not None:
            raise NotImplementedError("lr_config.warmup=%r (warmup is not built)"
                                      % (lrc.get("warmup"),))
        if not lrc.get("by_epoch", True):
            raise NotImplementedError("lr_config.by_epoch=False (the step policy is by epoch)")
        logc = cfg.get("log_config") or {}
        for hook in logc.get("hooks", [dict(type="TextLoggerHook")]):
            t = hook.get("type")
            if t == "WandbLoggerHook":
                warnings.warn("log_config.hooks: WandbLoggerHook skipped (no network)")
            elif t != "TextLoggerHook":
                raise NotImplementedError("log_config.hooks type=%r (built: TextLoggerHook)" % (t,))
        ck = dict(cfg.get("checkpoint_config") or {})
        if not ck.get("by_epoch", True):
            # (configs/mask2former/baseline_r50_psg.py:559 saves every 500 iterations)
            warnings.warn("checkpoint_config.by_epoch=False: checkpoints by iteration are not "
                          "built; one is written at every epoch's end instead")
            ck["interval"] = 1
        spg = int(get(cfg.get("data"), "samples_per_gpu", 2))
        world = 1
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            world = int(dist.get_world_size(kw.get("group")))
        trainer_kw = dict(kw.pop("trainer_kw", None) or {})
        opt = cfg.get("optimizer") or {}
        if "lr" in opt:
            trainer_kw.setdefault("lr", auto_scaled_lr(opt["lr"], cfg.get("auto_scale_lr"), world,
                                                       spg))
        if "weight_decay" in opt:
            trainer_kw.setdefault("weight_decay", float(opt["weight_decay"]))
        clip = get(cfg.get("optimizer_config"), "grad_clip")
        if clip and "max_norm" in clip:
            trainer_kw.setdefault("max_norm", float(clip["max_norm"]))
        args = dict(samples_per_gpu=spg, max_epochs=int(runner.get("max_epochs", 15)),
                    lr_steps=lrc.get("step", []), lr_gamma=float(lrc.get("gamma", 0.1)),
                    ckpt_interval=int(ck.get("interval", 1)),
                    max_keep_ckpts=int(ck.get("max_keep_ckpts", -1)),
                    log_interval=int(logc.get("interval", 50)),
                    resume_from=cfg.get("resume_from"), load_from=cfg.get("load_from"),
                    trainer_kw=trainer_kw)
        args.update(kw)
        return cls(det, args.pop("trainer", None), dataset, work_dir=work_dir, **args)

    # ------------------------------------------------------------------ set-up
    def _adopt(self, trainer):
        name = type(trainer).__name__
        if name not in ENTRIES:
            raise ValueError("no training step for a %s" % name)
        self.trainer = trainer
        self._row = TRAIN_ENTRIES[name]
        setattr(self.det, self._row.slot, trainer)     # the detector's step entry runs THIS trainer

    def _prepare(self):
        """`load_from` / `resume_from`, then the trainer; returns the meta to start from."""
        start = None
        kw = dict(self.trainer_kw)
        if self.group is not None:
            kw.setdefault("group", self.group)
        if self.resume_from:
            trainer, start = _restore(self.det, self.resume_from, kw)
            self._adopt(trainer)
        elif self.trainer is None:
            if self.load_from:
                load_checkpoint(self.det, self.load_from)
            name = HEAD_TRAINER.get(type(self.det.bbox_head).__name__)
            self._adopt(_build_trainer(self.det, name, kw))
        return start

    def _open_log(self):
        path = None
        if self.rank == 0:
            os.makedirs(self.work_dir, exist_ok=True)
            path = os.path.join(self.work_dir, time.strftime("%Y%m%d_%H%M%S") + ".log.json")
        self.log_path = path
        self.log = TrainLog(self.trainer.dev, self.log_interval, path)

    # ------------------------------------------------------------------ one iteration
    def _next_batch(self, order, pos):
        """-> (batch dict, the dataset indices it holds, the next position in `order`)."""
        first = self.dataset[order[pos]]
        if isinstance(first, dict):
            return first, [order[pos]], pos + 1
        if self.pipeline is None:
            raise ValueError("raw samples need pipeline= (a TrainPipeline)")
        idx = list(order[pos:pos + self.samples_per_gpu])
        samples = [first] + [self.dataset[i] for i in idx[1:]]
        for _ in range(100):
            batch = self.pipeline.batch(samples, rng=self.rng)
            if batch is not None:
                return batch, idx, pos + len(idx)
            for j in self.pipeline.rejected:      # mmdet's dataset: another image, at random
                idx[j] = int(self.rng.randint(len(self.dataset)))
                samples[j] = self.dataset[idx[j]]
        raise RuntimeError("no crop kept a relation in 100 draws (samples %s)" % idx)

    def _step(self, b):
        masks = (b.get("gt_masks"),) if self._row.masks else ()
        return getattr(self.det, self._row.step)(b["img"], b["img_metas"], b["gt_rels"],
                                                 b.get("gt_bboxes"), b["gt_labels"], *masks)

    def train_epoch(self, epoch, flush=True):
        """One epoch (0-based).  `flush=False` leaves the log's records in flight -- the loop then
        holds no host wait at all (`log.poll()` / `log.flush()` are the caller's)."""
        if self.log is None:
            self._open_log()
        tr = self.trainer
        lr = tr.set_epoch(epoch, self.lr_steps, self.lr_gamma)
        order = epoch_order(len(self.dataset), epoch, self.seed, self.rank, self.world, self.shuffle)
        pos, inner = 0, 0
        t0 = time.perf_counter()
        while pos < len(order):
            batch, idx, pos = self._next_batch(order, pos)
            t1 = time.perf_counter()
            self.handed.append((epoch, idx))
            out = self._step(batch)
            self.iter += 1
            inner += 1
            t2 = time.perf_counter()
            # (host times: the loop does not wait for the device, so `time` is what the host
            # spends per iteration -- the device's pace shows once the queue is full)
            self.log.add(out, epoch=epoch + 1, iter=inner, lr=lr, time=t2 - t0, data_time=t1 - t0)
            t0 = t2
        if flush:
            self.log.flush()
        else:
            self.log.close_window()
        self.epoch = epoch + 1

    # ------------------------------------------------------------------ checkpoints
    def meta(self):
        return dict(epoch=int(self.epoch), iter=int(self.iter), seed=int(self.seed),
                    runner=dict(pipeline_rng=_rng_state(self.rng), world=self.world,
                                samples_per_gpu=self.samples_per_gpu))

    def save(self):
        """`epoch_{n}.pth` (rank 0), pruning, `latest.pth`."""
        if self.rank != 0:
            return None
        os.makedirs(self.work_dir, exist_ok=True)
        name = "epoch_%d.pth" % self.epoch
        save_checkpoint(self.det, self.trainer, os.path.join(self.work_dir, name), self.meta())
        if self.max_keep_ckpts > 0:
            have = []
            for f in os.listdir(self.work_dir):
                if f.startswith("epoch_") and f.endswith(".pth") and f[6:-4].isdigit():
                    have.append((int(f[6:-4]), f))
            for _, f in sorted(have)[:-self.max_keep_ckpts]:
                os.remove(os.path.join(self.work_dir, f))
        link = os.path.join(self.work_dir, "latest.pth")
        tmp = link + ".tmp.%d" % os.getpid()
        if os.path.lexists(tmp):
            os.remove(tmp)
        os.symlink(name, tmp)                    # relative: the work_dir can be moved
        os.replace(tmp, link)
        return name

    # ------------------------------------------------------------------ the loop
    def run(self, start=None):
        """Train epochs [start's epoch, max_epochs).  `start`: a checkpoint's `meta` (as `resume`
        returns it) to continue from."""
        restored = self._prepare()
        start = start if start is not None else restored
        if start is not None:
            self.epoch, self.iter = int(start.get("epoch", 0)), int(start.get("iter", 0))
            r = start.get("runner") or {}
            if "pipeline_rng" in r:
                _set_rng_state(self.rng, r["pipeline_rng"])
        if self.log is None:
            self._open_log()
        for epoch in range(self.epoch, self.max_epochs):
            self.train_epoch(epoch)
            if self.ckpt_interval > 0 and self.epoch % self.ckpt_interval == 0:
                self.save()
        return self
