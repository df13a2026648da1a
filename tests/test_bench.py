"""bench.py's contract: `--dump-outputs DIR` writes the result tuples of the last timed step
(float32 / float64 .npy files, a seeded sample of the large fields, a few MB in all), and a
plain run does the headline only -- the secondary legs and figures come with `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_results(B=2, R=100, H0=384, W0=640, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(B):
        out.append((torch.zeros(2 * R, 5), torch.randint(1, 134, (2 * R,), generator=g),
                    torch.arange(2 * R, dtype=torch.int).reshape(2, -1).T,
                    torch.rand(2 * R, H0, W0, generator=g) > 0.5,
                    torch.randint(0, 1 << 20, (H0, W0), generator=g),
                    torch.zeros(R), torch.zeros(R), torch.rand(R, 57, generator=g)))
    return out


def test_dump_outputs_writes_every_field_in_float_within_budget(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    res = _fake_results()
    names = bench.dump_outputs(str(tmp_path / "a"), res)
    assert names == sorted(["refine_bboxes", "labels", "rel_pair_idxes", "masks_sample",
                            "masks_area", "pan_results", "rel_scores", "rel_labels", "rel_dists"])
    total = 0
    for n in names:
        a = np.load(tmp_path / "a" / (n + ".npy"))
        assert a.dtype in (np.float32, np.float64), n
        total += a.nbytes
    assert total <= 64 << 20
    # whole fields are exact; the masks are a fixed sample plus their exact areas
    labels = np.load(tmp_path / "a" / "labels.npy")
    assert np.array_equal(labels, torch.stack([r[1] for r in res]).numpy().astype(np.float64))
    pan = np.load(tmp_path / "a" / "pan_results.npy")
    assert np.array_equal(pan, torch.stack([r[4] for r in res]).numpy().astype(np.float64))
    area = np.load(tmp_path / "a" / "masks_area.npy")
    assert np.array_equal(area, torch.stack([r[3] for r in res]).flatten(2).sum(-1).numpy())
    assert np.load(tmp_path / "a" / "masks_sample.npy").shape == (bench.DUMP_SAMPLE,)
    # same results -> the same files (the sample positions are fixed)
    bench.dump_outputs(str(tmp_path / "b"), res)
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / (n + ".npy")),
                              np.load(tmp_path / "b" / (n + ".npy"))), n


def test_dump_outputs_box_trunk_tuple(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    R = 100
    res = [(torch.rand(2 * R, 5), torch.randint(1, 134, (2 * R,)), torch.randint(0, 100, (R, 2)),
            torch.rand(R), torch.randint(1, 57, (R,)), torch.rand(R, 57))]
    names = bench.dump_outputs(str(tmp_path), res)
    assert names == sorted(bench.RESULT_FIELDS[6])
    assert np.load(tmp_path / "rel_dists.npy").dtype == np.float32
    assert np.load(tmp_path / "rel_pair_idxes.npy").shape == (1, R, 2)


@pytest.mark.gpu
def test_plain_bench_run_times_k_steps_and_dumps_the_last_step(tmp_path):
    """A plain run at a small size: exactly K timed steps, `ms_per_step` on the line, none of
    the --full figures, and the dumped outputs identical across two runs with the same
    arguments."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    recs = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7",
               "--warmup", "2", "--height", "256", "--width", "320",
               "--dump-outputs", str(tmp_path / run)]
        out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=400)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        recs.append(json.loads(lines[0]))
    for rec in recs:
        assert rec["steps"] == 7 and rec["warmup"] == 2 and rec["value"] > 0
        assert rec["ms_per_step"] > 0 and rec["unit"] == "images/s" and rec["dtype"] == "f32"
        assert rec["higher_is_better"] is True
        for k in ("roofline", "kernel_profile", "cpu_baseline", "head_only", "box_trunk"):
            assert k not in rec, k
        assert rec["pipeline_check"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    assert "labels.npy" in names and "masks_sample.npy" in names and "pan_results.npy" in names
    assert names == sorted(os.listdir(tmp_path / "b"))
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
