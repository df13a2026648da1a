"""CPU: the parts of pair-net_amd/runner.py that need no GPU -- `epoch_order` against
`torch.utils.data.DistributedSampler`, `EpochRunner.from_config` on the restated and the reference's
own config files, the auto-scaled learning rate, every refusal, and the two log entries of the C
ABI."""
import os
import re
import warnings

import pytest
import torch
from torch.utils.data import DistributedSampler

from oracle import ref_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("N", [1, 5, 8, 13])
def test_epoch_order_is_the_distributed_samplers(N, world, shuffle):
    from pairnet_amd import epoch_order
    seed = 10086
    for rank in range(world):
        sampler = DistributedSampler(range(N), num_replicas=world, rank=rank, shuffle=shuffle,
                                     seed=seed)
        for e in (0, 1, 7):
            sampler.set_epoch(e)
            assert epoch_order(N, e, seed, rank, world, shuffle) == list(sampler.__iter__()), \
                (N, world, rank, e, shuffle)
    with pytest.raises(ValueError):
        epoch_order(N, 0, seed, world, world)


def _check_pairnet(r):
    assert r.max_epochs == 15 and r.lr_steps == (5, 10) and r.lr_gamma == 0.5
    assert r.log_interval == 50 and r.max_keep_ckpts == 15 and r.ckpt_interval == 1
    assert r.samples_per_gpu == 2 and r.seed == 10086 and r.trainer is None
    # world 1, 2 per GPU, base batch 8: 1e-4 * 2 / 8
    assert r.trainer_kw["lr"] == pytest.approx(2.5e-5, rel=1e-12)
    assert r.trainer_kw["weight_decay"] == 1e-4 and r.trainer_kw["max_norm"] == 0.1
    assert r.load_from == "pretrain/m2f_r50_coco.pth" and r.resume_from is None


def test_from_config_on_the_restated_config(tmp_path):
    from pairnet_amd import EpochRunner, build_detector, pairnet_r50
    cfg = pairnet_r50(schedule=True)
    assert dict(cfg.model) == dict(pairnet_r50())
    det = build_detector(cfg.model)
    r = EpochRunner.from_config(cfg, det, [None] * 4, str(tmp_path))
    _check_pairnet(r)
    assert r.work_dir == str(tmp_path) and not os.listdir(tmp_path)      # nothing written yet
    r = EpochRunner.from_config(cfg, det, [None] * 4, str(tmp_path), seed=3, max_epochs=2)
    assert r.seed == 3 and r.max_epochs == 2


@pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")
def test_from_config_on_the_references_files(tmp_path):
    from pairnet_amd import EpochRunner, build_detector, load_config, pairnet_r50
    cfg = load_config(os.path.join(ref_shim.REF_ROOT, "configs/mask2former/pairnet.py"))
    restated = pairnet_r50(schedule=True)
    for k in ("optimizer", "optimizer_config", "lr_config", "runner", "checkpoint_config",
              "log_config", "auto_scale_lr", "load_from"):
        assert cfg[k] == restated[k], k
    assert cfg["data"]["samples_per_gpu"] == restated["data"]["samples_per_gpu"]
    det = build_detector(dict(cfg.model))
    _check_pairnet(EpochRunner.from_config(cfg, det, [None] * 4, str(tmp_path)))
    base = load_config(os.path.join(ref_shim.REF_ROOT, "configs/_base_/custom_runtime.py"))
    assert base["checkpoint_config"] == dict(interval=1, max_keep_ckpts=1)
    assert base["log_config"]["interval"] == 50 and base["resume_from"] is None
    # the sibling head's file: 12 epochs, one step at 40 with mmcv's default gamma, checkpoints by
    # iteration (not built: written at the epoch's end, with a warning)
    cfg = load_config(os.path.join(ref_shim.REF_ROOT, "configs/mask2former/baseline_r50_psg.py"))
    det = build_detector(dict(cfg.model))
    with pytest.warns(UserWarning, match="by_epoch=False"):
        r = EpochRunner.from_config(cfg, det, [None] * 4, str(tmp_path))
    assert r.max_epochs == 12 and r.lr_steps == (40,) and r.lr_gamma == 0.1
    assert r.log_interval == 50 and r.max_keep_ckpts == 15 and r.ckpt_interval == 1
    assert r.trainer_kw["lr"] == pytest.approx(2.5e-5, rel=1e-12)


def test_auto_scaled_lr():
    from pairnet_amd.runner import auto_scaled_lr
    on = dict(enable=True, base_batch_size=8)
    assert auto_scaled_lr(1e-4, on, 1, 2) == pytest.approx(1e-4 * 2 / 8, rel=1e-12)
    assert auto_scaled_lr(1e-4, on, 4, 2) == pytest.approx(1e-4, rel=1e-12)
    assert auto_scaled_lr(1e-4, dict(enable=False, base_batch_size=8), 1, 2) == 1e-4
    assert auto_scaled_lr(1e-4, None, 1, 2) == 1e-4
    with pytest.raises(ValueError, match="base_batch_size"):
        auto_scaled_lr(1e-4, dict(enable=True), 1, 2)


def test_refusals_name_their_key(tmp_path):
    from pairnet_amd import EpochRunner, build_detector, pairnet_r50
    det = build_detector(pairnet_r50())

    def make(**over):
        cfg = pairnet_r50(schedule=True)
        cfg.update(over)
        return EpochRunner.from_config(cfg, det, [None] * 4, str(tmp_path))
    with pytest.raises(NotImplementedError, match="lr_config.policy"):
        make(lr_config=dict(policy="CosineAnnealing", min_lr=0))
    with pytest.raises(NotImplementedError, match="lr_config.warmup"):
        make(lr_config=dict(policy="step", step=[5, 10], warmup="linear", warmup_iters=500))
    with pytest.raises(NotImplementedError, match="runner.type.*IterBasedRunner"):
        make(runner=dict(type="IterBasedRunner", max_iters=1000))
    with pytest.raises(NotImplementedError, match="log_config.hooks.*TensorboardLoggerHook"):
        make(log_config=dict(interval=50, hooks=[dict(type="TextLoggerHook"),
                                                 dict(type="TensorboardLoggerHook")]))
    with pytest.warns(UserWarning, match="WandbLoggerHook"):
        r = make(log_config=dict(interval=20, hooks=[dict(type="TextLoggerHook"),
                                                     dict(type="WandbLoggerHook")]))
    assert r.log_interval == 20
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # the plain config warns about nothing
        make()
    with pytest.raises(ValueError, match="trainer=None"):
        EpochRunner(det, object(), [None], work_dir=str(tmp_path), resume_from="x.pth")


def test_batches_from_raw_samples_and_the_pipeline_generator(tmp_path):
    """`dataset[i]` as a raw sample goes through `pipeline.batch` with the runner's generator,
    `samples_per_gpu` at a time, the last batch short; a rejected crop draws another image; a
    ready batch dict is one iteration by itself.  The generator's state survives a
    `weights_only` file."""
    import numpy as np
    from pairnet_amd import EpochRunner, epoch_order
    from pairnet_amd.runner import _rng_state, _set_rng_state

    class Pipe:
        calls, rejected = 0, []

        def batch(self, samples, rng=None):
            assert rng is not None
            self.calls += 1
            self.rejected = [1] if self.calls == 1 else []
            return None if self.rejected else dict(samples=list(samples))
    data = [("sample", i) for i in range(5)]
    r = EpochRunner(None, None, data, pipeline=Pipe(), samples_per_gpu=2, seed=1,
                    work_dir=str(tmp_path))
    order = epoch_order(5, 0, 1)
    b, idx, pos = r._next_batch(order, 0)
    assert pos == 2 and r.pipeline.calls == 2 and idx[0] == order[0] and 0 <= idx[1] < 5
    assert b["samples"] == [data[idx[0]], data[idx[1]]]
    b, idx, pos = r._next_batch(order, 4)                            # drop_last=False
    assert pos == 5 and idx == [order[4]] and b["samples"] == [data[order[4]]]
    with pytest.raises(ValueError, match="pipeline="):
        EpochRunner(None, None, data, work_dir=str(tmp_path))._next_batch(order, 0)
    ready = [dict(img=i) for i in range(3)]
    r2 = EpochRunner(None, None, ready, samples_per_gpu=2, work_dir=str(tmp_path))
    assert r2._next_batch([2, 0, 1], 1) == (ready[0], [0], 2)
    # the pipeline generator through a checkpoint's meta
    r.rng.randint(10, size=7)
    path = str(tmp_path / "meta.pth")
    torch.save(dict(meta=r.meta()), path)
    meta = torch.load(path, weights_only=True)["meta"]
    assert meta["epoch"] == 0 and meta["seed"] == 1
    want = r.rng.randint(1 << 30, size=5)
    other = np.random.RandomState(0)
    _set_rng_state(other, meta["runner"]["pipeline_rng"])
    assert np.array_equal(other.randint(1 << 30, size=5), want)
    assert _rng_state(other)["pos"] == _rng_state(r.rng)["pos"]


def test_trainer_state_refuses_a_mismatch_by_name():
    """`FlatTrainer.load_state_dict` checks before it writes (no GPU: a bare object with the
    attributes the check reads)."""
    from pairnet_amd.flat_trainer import FlatTrainer

    class T(FlatTrainer):
        def __init__(self):
            self.names = ["a.weight", "b.bias"]
            self.layout = {"a.weight": (0, (2, 3), 6), "frozen": (6, (2,), 2), "b.bias": (8, (4,), 4)}
    t = T()
    state = {i: dict(step=torch.tensor(1.0), exp_avg=torch.zeros(s), exp_avg_sq=torch.zeros(s))
             for i, s in enumerate([(2, 3), (4,)])}
    block = {"class": "T", "steps": 1, "lr": 1e-4, "base_lr": 1e-4}
    sd = dict(optimizer=dict(state=state, param_names=["a.weight", "b.bias"]), trainer=block)
    with pytest.raises(ValueError, match="TailTrainer"):
        t.load_state_dict(dict(sd, trainer=dict(block, **{"class": "TailTrainer"})))
    with pytest.raises(ValueError, match="entry 1.*'c.bias'"):
        t.load_state_dict(dict(sd, optimizer=dict(state=state, param_names=["a.weight", "c.bias"])))
    bad = {0: state[0], 1: dict(state[1], exp_avg_sq=torch.zeros(5))}
    with pytest.raises(ValueError, match="exp_avg_sq of b.bias"):
        t.load_state_dict(dict(sd, optimizer=dict(state=bad, param_names=["a.weight", "b.bias"])))


def test_header_carries_the_two_log_entries():
    from pairnet_amd import build as B
    from pairnet_amd import hip
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    for name in ("pn_train_log_row_f32", "pn_train_log_window_f32"):
        assert name in declared and name in hip._SIGS and name in hip.EXPORTS, name
    assert "#define PN_ABI_VERSION 34" in header and hip.ABI_VERSION == 34
    assert len(hip._SIGS["pn_train_log_row_f32"][1]) == 10
    assert len(hip._SIGS["pn_train_log_window_f32"][1]) == 7
    assert "TextLoggerHook" in header and "LogBuffer.average" in header
    assert "train_log" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "train_log.hip"))
    assert callable(hip.train_log_row) and callable(hip.train_log_window)
    assert hip.LOG_MAX_TERMS == 32
