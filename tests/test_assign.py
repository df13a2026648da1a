"""CPU: the assignment algorithm csrc/assign.hip implements, restated in Python (tests/lsa_ref.py),
equals `scipy.optimize.linear_sum_assignment` pair for pair -- ties included -- on seeded problems;
the C ABI declares the new entries at version 33; the new source compiles for gfx950 without scratch.
The kernel itself is compared with scipy on the GPU (tests/test_assign_gpu.py)."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import lsa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("ints", "dup", "random")


def _same(cost):
    want_r, want_c = linear_sum_assignment(cost.astype(np.float64))
    got_r, got_c, st = lsa_ref.lsa(cost)
    assert st == 0
    assert np.array_equal(got_r, want_r) and np.array_equal(got_c, want_c), (cost.shape, got_c, want_c)


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_equals_scipy_on_small_problems(kind):
    rng = np.random.default_rng(KINDS.index(kind))
    for _ in range(400):
        rows, cols = rng.integers(1, 14, 2)
        _same(lsa_ref.problems(kind, int(rows), int(cols), rng))


def test_restatement_equals_scipy_on_query_sized_problems_with_duplicated_columns():
    rng = np.random.default_rng(7)
    for T in (1, 2, 5, 12, 20, 37, 60):
        _same(lsa_ref.problems("dup", 100, T, rng))
        _same(lsa_ref.problems("ints", 100, T, rng))
    # the fixture's own tie (tests/test_losses_gpu.py: relations [0,1,5] and [0,1,9] share a class
    # pair and r_cls_cost's weight is 0): bit-identical columns
    c = rng.standard_normal((100, 5)).astype(np.float32)
    c[:, 4] = c[:, 0]
    _same(c)


def test_restatement_equals_scipy_on_single_rows_and_columns():
    rng = np.random.default_rng(8)
    for n in (1, 2, 7, 64, 65):
        for kind in KINDS:
            _same(lsa_ref.problems(kind, 1, n, rng))
            _same(lsa_ref.problems(kind, n, 1, rng))


def test_restatement_reports_what_scipy_raises_on():
    c = np.ones((4, 3), np.float32)
    for bad, status in ((np.nan, 1), (-np.inf, 1)):
        d = c.copy()
        d[2, 1] = bad
        with pytest.raises(ValueError):
            linear_sum_assignment(d)
        r, cc, st = lsa_ref.lsa(d)
        assert st == status and (r == -1).all() and (cc == -1).all() and len(r) == 3
    d = c.copy()
    d[:, 1] = np.inf                      # transposed problem: a row of +inf
    with pytest.raises(ValueError):
        linear_sum_assignment(d)
    assert lsa_ref.lsa(d)[2] == 2
    d = np.ones((3, 4), np.float32)
    d[1, :] = np.inf
    with pytest.raises(ValueError):
        linear_sum_assignment(d)
    assert lsa_ref.lsa(d)[2] == 2
    d = np.ones((3, 4), np.float32)
    d[1, 2] = np.inf                      # a single +inf entry is ordinary data
    _same(d)


def test_header_and_binding_declare_the_new_entries():
    from pairnet_amd import build as B
    from pairnet_amd import hip
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    for name in ("pn_lsa_f32", "pn_loss_targets", "pn_adamw_guarded_f32"):
        assert name in declared and name in hip._SIGS and name in hip.EXPORTS, name
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION == 34
    # the existing optimizer entry keeps its argument list (the betas are doubles from ABI 34); the
    # guarded one adds the status word
    assert len(hip._SIGS["pn_adamw_f32"][1]) == 18 and len(hip._SIGS["pn_adamw_guarded_f32"][1]) == 19
    assert callable(hip.lsa) and callable(hip.loss_targets) and "assign" in B.SOURCES
    for cite in ("matcher.py:262-264", "mask_hungarian_assigner.py", "pairnet_head.py:645-718"):
        assert cite in header, cite


def test_bad_arguments_are_refused_without_launching(built_lib):
    from pairnet_amd import hip
    lib = hip.lib()
    assert lib.pn_lsa_f32(None, 4, None, 1, 0, None, None, 1, None, None) == -1
    assert lib.pn_loss_targets(*([None] * 6), 1, 1, 100, 100, 56, *([None] * 5)) == -1
    assert lib.pn_adamw_guarded_f32(*([None] * 4), 4, None, None, None, 1, 1e-4, 0.9, 0.999, 1e-8,
                                    1e-4, 1, None, 1.0, None, None) == -1


def test_assign_kernels_compile_for_gfx950_without_scratch(tmp_path):
    from pairnet_amd import build as B
    out = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(B.CSRC, "assign.hip"), "-o", str(tmp_path / "assign.o")],
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
    kernels = {k: v for k, v in res.items() if "k_lsa" in k or "k_loss_targets" in k}
    assert len(kernels) == 2, sorted(res)
    for k, use in kernels.items():
        print(k, use)
        assert use["ScratchSize [bytes/lane]"] == 0, k
        # static LDS of the solver's state: 3 x 1024 doubles + 6 x 1024 ints; with the 96 KB of
        # staged costs the workgroup stays inside the CU's 160 KB
        assert use["LDS Size [bytes/block]"] <= 48 * 1024, k
