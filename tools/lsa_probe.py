"""Kernel time of `pn_lsa_f32` (csrc/assign.hip) on one MI355X next to
`scipy.optimize.linear_sum_assignment` on the same matrices on the host (labnotes/r11.md).

Per shape: one problem per launch, costs staged in LDS (the default) and read from memory
(`max_cells=0`), and a launch of four such problems (a batch of two images solves 2B = 4); device
events around windows of back-to-back launches long enough to exceed 100 ms; scipy timed over the
same number of calls including its float64 conversion (what `linear_sum_assignment(cost.numpy())`
does), without the device-to-host copy it needs in a training step.  Matrices: standard normal
fp32 ("random") and the id matcher's kind with duplicated columns ("dup").  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

import lsa_ref  # noqa: E402
from pairnet_amd import hip  # noqa: E402

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
SHAPES = [(100, 12), (100, 20), (100, 100), (200, 60)]
rng = np.random.default_rng(0)


def window(fn, min_ms=120.0):
    """us per call of `fn` from device events around a window of at least `min_ms`."""
    n = 64
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= min_ms:
            return 1e3 * ms / n, n
        n = int(n * max(2.0, 1.3 * min_ms / max(ms, 1e-3)))


def launcher(costs, max_cells):
    table, c_off, o_off = [], 0, 0
    for c in costs:
        table.append([c_off, c.shape[0], c.shape[1], o_off])
        c_off += c.size
        o_off += min(c.shape)
    flat = torch.from_numpy(np.concatenate([c.ravel() for c in costs])).to(dev)
    tab = torch.tensor(table, dtype=torch.int64, device=dev)
    rows = torch.empty(o_off, dtype=torch.int32, device=dev)
    cols = torch.empty_like(rows)
    status = torch.empty(len(costs), dtype=torch.int32, device=dev)
    return (lambda: hip.lsa(flat, tab, rows, cols, status, max_cells=max_cells)), rows, cols, status


out = {"what": "pn_lsa_f32, us per launch (device events, windows >= 120 ms) and scipy us per "
               "call on the host, same matrices"}
for kind in ("random", "dup"):
    for r, c in SHAPES:
        cost = lsa_ref.problems(kind, r, c, rng)
        rec = {}
        fn, rows, cols, status = launcher([cost], cost.size)
        rec["staged_us"], rec["launches"] = window(fn)
        want = linear_sum_assignment(cost.astype(np.float64))
        assert int(status.cpu()[0]) == 0 and np.array_equal(rows.cpu().numpy(), want[0]) \
            and np.array_equal(cols.cpu().numpy(), want[1])
        fn, rows, cols, status = launcher([cost], 0)
        rec["from_memory_us"], _ = window(fn)
        assert np.array_equal(cols.cpu().numpy(), want[1])
        four = [cost] + [lsa_ref.problems(kind, r, c, rng) for _ in range(3)]
        fn, rows, cols, status = launcher(four, cost.size)
        rec["four_problems_us"], _ = window(fn)
        n = rec["launches"]
        t0 = time.perf_counter()
        for _ in range(n):
            linear_sum_assignment(cost.astype(np.float64))
        rec["scipy_us"] = 1e6 * (time.perf_counter() - t0) / n
        out["%s %dx%d" % (kind, r, c)] = {k: round(v, 2) if isinstance(v, float) else v
                                          for k, v in rec.items()}
print(json.dumps(out))
