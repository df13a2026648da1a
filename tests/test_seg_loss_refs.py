"""CPU: (1) the float64 statements of tests/seg_loss_ref.py equal, to 1e-12, the functions they
restate -- torch's BCE-with-logits, `oracle.mmdet_train`'s DiceCost diagonal and
weight_reduce_loss, float64 autograd, the host Philox -- and, where the reference tree is present, the
reference's OWN `MaskFormerHead.loss` / `loss_single` / `_get_target_single` and
`get_uncertain_point_coords_with_randomness`, executed in place under name-only stubs
(tools/make_seg_loss_golden.py) with `torch.rand` handing out the injected draws; (2) the planted
conditions of the GPU cases hold: every assignment leads by far more than the match-cost bound of
labnotes R14.2, every selection case keeps the same k-set in fp32 as in float64; (3) the C ABI
declares the new entries, refuses bad arguments without launching, and csrc/seg_loss.hip compiles
for gfx950 without scratch.  The kernels run in tests/test_seg_loss_gpu.py."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_ref
import loss_optim_ref as R
import seg_loss_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle import ref_shim  # noqa: E402

NEW = ("pn_uniform_f32", "pn_seg_targets", "pn_uncertain_points_f32", "pn_point_sample_rows_f32",
       "pn_mask_point_loss_f32", "pn_point_scatter_grad_f32", "pn_ce_avg_f32", "pn_ce_avg_grad_f32")
need_ref = pytest.mark.skipif(not ref_shim.available(), reason="reference tree absent")


def _xt(M, Np, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, Np, generator=g) * 3.0
    t = torch.rand(M, Np, generator=g).round() * torch.rand(M, Np, generator=g)
    return x, t


# ---------------------------------------------------------------- (1) the statements are pinned
@need_ref
@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_equals_the_references_own_loss_in_float64(name):
    case, _ = S.golden_case(name)
    out, g_cls, g_mask = S.run_reference(case, torch.float64)
    r = S.run_whole(case)
    assert set(out) == set(r["losses"]) and len(out) == 3 * case["cls"].shape[0]
    for k in out:
        assert abs(float(out[k]) - float(r["losses"][k])) <= 1e-12, k
    assert float((g_cls - r["g_cls"]).abs().max()) <= 1e-12
    h, w = case["mask"].shape[-2:]
    dense = torch.zeros_like(g_mask).view(-1, h, w)
    dense[r["mask_rows"]] = r["g_mask"]          # every other row of the reference's gradient is 0
    assert float((g_mask.view(-1, h, w) - dense).abs().max()) <= 1e-12
    assert name != "a" or (float(out["loss_cls"]) > 0 and r["matched"].shape[0] == 6)


@need_ref
def test_selection_equals_the_references_point_sample_py():
    S.load_reference()
    fn = sys.modules["pairnet.models.panoptic_heads.point_sample"].get_uncertain_point_coords_with_randomness
    maps, cand = S.selection_case(5, 13, 21, 150, 1)
    tail = torch.rand(5, 13, 2, generator=torch.Generator().manual_seed(9))
    with S.injected_rand([cand, tail], torch.float64):
        got = fn(maps.double().unsqueeze(1), None, 50, 3.0, 0.75)
    pts, kept, _ = S.uncertain_points(maps, torch.arange(5), cand, tail, 37)
    assert got.shape == (5, 50, 2)
    for m in range(5):       # the reference keeps topk's order, the kernel ascending candidate order
        a = sorted(map(tuple, got[m, :37].tolist()))
        assert a == sorted(map(tuple, pts[m, :37].double().tolist()))
    assert torch.equal(got[:, 37:], pts[:, 37:].double())


@need_ref
def test_fixture_holds_what_the_reference_computes_in_fp32():
    for name in ("a", "b"):
        case, ref = S.golden_case(name)
        out, g_cls, g_mask = S.run_reference(case, torch.float32)
        got = np.array([float(out[k]) for k in ref["names"]], np.float32)
        assert np.array_equal(got, ref["loss32"]) and np.array_equal(g_cls.numpy(), ref["g_cls32"])


def test_fixture_holds_the_restatements_float64_values():
    for name in ("a", "b"):
        case, ref = S.golden_case(name)
        r = S.run_whole(case)
        for k, v in zip(ref["names"], ref["loss64"]):
            assert abs(float(r["losses"][str(k)]) - v) <= 1e-12
        assert np.array_equal(r["matched"].numpy(), ref["matched"])
        scale = S.U * (r["g_mask_mag"] + S.COORD * r["g_mask_coord"]).numpy() + S.FLT_MIN
        assert (np.abs(ref["g_mask32"] - r["g_mask"].numpy()) <= (float(ref["g_mask_ratio"]) + 1e-6) * scale).all()
        scale = S.U * r["g_cls_mag"].numpy() + S.FLT_MIN
        assert (np.abs(ref["g_cls32"] - r["g_cls"].numpy()) <= (float(ref["g_cls_ratio"]) + 1e-6) * scale).all()
        # the stored fp32 reference is within its own stored ratio of the float64 values
        err = np.abs(ref["loss32"].astype(np.float64) - ref["loss64"])
        assert (err <= (ref["loss_ratio"] + 1e-6) * S.U * ref["loss_mag"] + S.FLT_MIN).all()


def test_bce_dice_and_reduction_equal_torch_and_the_oracle(monkeypatch):
    from oracle.mmdet_train import DiceCost, weight_reduce_loss
    x, t = _xt(6, 50, 3)
    x64, t64 = x.double(), t.double()
    want = F.binary_cross_entropy_with_logits(x64, t64, reduction="none")
    assert float((S.bce(x64, t64) - want).abs().max()) <= 1e-12
    r = S.mask_point_loss(x, t, torch.ones(6, dtype=torch.bool), 2, 5.0, 3.0, 1.0)
    # (DiceCost casts its targets with `.float()`: let the cast follow the float64 run)
    monkeypatch.setattr(torch.Tensor, "float", lambda self, *a, **k: self.double())
    dice = torch.diagonal(DiceCost(weight=1.0, pred_act=True, eps=1.0)(x64, t64))
    monkeypatch.undo()
    for l in range(2):
        sl = slice(3 * l, 3 * l + 3)
        n = torch.tensor(3.0, dtype=torch.float64)
        assert abs(float(r["mask"][l]) - 5.0 * float(weight_reduce_loss(want[sl].reshape(-1), None, "mean", n * 50))) <= 1e-12
        assert abs(float(r["dice"][l]) - 3.0 * float(weight_reduce_loss(dice[sl], None, "mean", n))) <= 1e-12
    # an explicit num_total_masks replaces the count; unassigned rows drop out
    v = torch.tensor([1, 0, 1, 1, 1, 1], dtype=torch.bool)
    r2 = S.mask_point_loss(x, t, v, 2, 5.0, 3.0, 1.0)
    assert abs(float(r2["mask"][0]) - 5.0 * float(want[[0, 2]].sum() / (2 * 50 + S.EPS32))) <= 1e-12
    r3 = S.mask_point_loss(x, t, v, 2, 5.0, 3.0, 1.0, ntm=2.5)
    assert abs(float(r3["dice"][1]) - 3.0 * float(dice[3:].sum() / (2.5 + S.EPS32))) <= 1e-12


def test_coefficients_equal_the_kernels_formula_and_ce_avg_equals_the_oracle():
    from oracle.mmdet_train import cross_entropy
    x, t = _xt(6, 50, 4)
    valid = torch.tensor([1, 1, 0, 1, 1, 1], dtype=torch.bool)
    coef, mag = S.mask_point_coef(x, t, valid, 2, 5.0, 3.0, 1.0)
    r = S.mask_point_loss(x, t, valid, 2, 5.0, 3.0, 1.0)
    s, tt, sm = torch.sigmoid(x.double()), t.double(), r["sums"]
    num, den = (2 * sm[:, 1] + 1.0)[:, None], (sm[:, 2] + sm[:, 3] + 1.0)[:, None]
    lay = torch.arange(6) // 3
    want = 5.0 * (s - tt) / r["den"][lay, 0][:, None] + \
        (3.0 / r["den"][lay, 1][:, None]) * ((num - 2 * tt * den) / (den * den)) * s * (1 - s)
    want = want * valid[:, None]
    assert float((coef - want).abs().max()) <= 1e-12 and bool((mag >= want.abs() - 1e-15).all())
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(2, 16, 6, generator=g) * 3
    y = torch.randint(0, 6, (2, 16), generator=g)
    cw = [1.0] * 5 + [0.1]
    got, _ = S.ce_avg(logits, y, cw, 2.0)
    cwt = torch.tensor(cw).double()
    for l in range(2):
        want = 2.0 * cross_entropy(logits[l].double(), y[l], class_weight=cwt, reduction="mean",
                                   avg_factor=cwt[y[l]].sum())
        assert abs(float(got[l]) - float(want)) <= 1e-12


def test_scatter_is_the_transpose_of_the_sample():
    g = torch.Generator().manual_seed(6)
    maps = torch.randn(3, 13, 21, generator=g)
    pts = torch.rand(3, 50, 2, generator=g)
    pts[0, 0], pts[0, 1] = torch.tensor([0.0, 0.0]), torch.tensor([1.0, float(np.nextafter(np.float32(1), np.float32(0)))])
    coef = torch.randn(3, 50, generator=g)
    m = maps.double().requires_grad_(True)
    (S.sample_rows(m, torch.arange(3), pts) * coef.double()).sum().backward()
    out, mag, cnt, coord = S.scatter(coef, pts, 13, 21)
    assert float((out - m.grad).abs().max()) <= 1e-12
    assert bool((mag >= out.abs() - 1e-15).all()) and bool((coord >= mag).all()) and float(cnt.sum()) <= 4 * 150
    # and the sample itself equals grid_sample
    want = F.grid_sample(maps.double()[:, None], (2.0 * pts.double() - 1.0)[:, :, None, :],
                         align_corners=False)[:, 0, :, 0]
    assert float((S.sample_rows(maps, torch.arange(3), pts) - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099])
def test_uniform_is_the_host_philox(n):
    u = S.uniform(n, 0x123456789ABCDEF, 3, 7, 11)
    j = np.arange((n + 3) // 4, dtype=np.uint64)
    words = np.stack(dropout_ref.philox4x32_10((j, 3, 7, 11), (0x89ABCDEF, 0x1234567)), 1).reshape(-1)[:n]
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, (words >> np.uint64(8)).astype(np.float64))
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    if n >= 4:
        for other in ((1, 3, 7, 11), (0x123456789ABCDEF, 4, 7, 11), (0x123456789ABCDEF, 3, 8, 11),
                      (0x123456789ABCDEF, 3, 7, 12)):
            assert not np.array_equal(u, S.uniform(n, *other))


# ---------------------------------------------------------------- (2) planted conditions
def _whole_cases():
    for name in ("a", "b"):
        yield name, S.golden_case(name)[0], None
    for name, shape in S.WHOLE_CASES.items():
        c = S.loss_case(**shape)
        yield name, c, c["planted"]


def test_every_assignment_case_leads_by_more_than_the_match_cost_bound():
    for name, case, planted in _whole_cases():
        r = S.run_whole(case)
        r32 = S.run_whole(case, dtype=torch.float32)
        Np, C1 = case["num_points"], case["cls"].shape[-1]
        h, w = case["mask"].shape[-2:]
        for key, cost in r["costs"].items():
            rows = r["matched"][(r["matched"][:, 0] == key[0]) & (r["matched"][:, 1] == key[1])]
            goff = sum(int(g.shape[0]) for g in case["gt_labels"][:key[1]])
            pairs = sorted((int(q), int(g) - goff) for _, _, q, g in rows.tolist())
            if planted is not None:
                assert pairs == planted[key], (name, key)
            margin = R.assignment_margin(cost, *zip(*pairs))
            # R14.2, generously: the largest chain (dice: 2 K + 11, class: 14 + z <= 102) + 2 + 4 on
            # an over-estimate of the three terms' magnitudes (2 + 5 * 100 + 10), twice the torch
            # fp32 oracle's own error, and the samples' error (18 roundings of (1 + max(h, w)) max|tap|)
            # carried through the mask cost (Lipschitz 5) and the dice cost (<= 10)
            K = math.ceil(Np / 256) + 10
            a = 2.0 * float((r32["costs"][key].double() - cost).abs().max())
            bound = (max(2 * K + 11, 102) + 6) * S.U * 512.0 + a + \
                18 * S.U * (1 + max(h, w)) * float(case["mask"].abs().max()) * 15.0
            assert 2 * bound < margin.min() and margin.min() > 1e-3, (name, key, bound, margin.min())
        assert name != "g_gt_q" or r["matched"].shape[0] == 2 * (4 + 2)
        assert name != "empty" or r["matched"].shape[0] == 0


def test_every_selection_case_keeps_the_same_set_in_fp32_and_float64():
    for Sn, k, seed in S.SELECTION_CASES:
        maps, cand = S.selection_case(5, 13, 21, Sn, seed)
        idx = torch.arange(5)
        _, kept64, key64 = S.uncertain_points(maps, idx, cand, None, k)
        _, kept32, _ = S.uncertain_points(maps, idx, cand, None, k, torch.float32)
        assert torch.equal(kept64, kept32), (Sn, k, seed)
        if 0 < k < Sn:
            # separated: the gap around the k-th value exceeds the point-sample bound on both sides
            srt = torch.sort(key64, 1)[0]
            gap = (srt[:, k] - srt[:, k - 1]).min()
            assert float(gap) > 2 * 18 * S.U * float(S.sample_mag(maps, idx).max()), (Sn, k, seed)
    for name, case, _ in _whole_cases():
        if name != "empty":
            assert torch.equal(S.run_whole(case)["kept"], S.run_whole(case, dtype=torch.float32)["kept"]), name


# ---------------------------------------------------------------- (3) ABI, refusals, compile
def test_header_and_binding_declare_the_new_entries():
    from pairnet_amd import build as B
    from pairnet_amd import hip
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    for name in NEW + ("pn_point_scatter_scratch_ints",):
        assert name in declared and name in hip._SIGS and name in hip.EXPORTS, name
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION == 34
    assert "seg_loss" in B.SOURCES
    for fn in ("uniform", "seg_targets", "uncertain_points", "point_sample_rows", "mask_point_loss",
               "point_scatter_grad", "ce_avg", "ce_avg_grad"):
        assert callable(getattr(hip, fn)), fn
    for cite in ("mask2former_head.py:157-324", "maskformer_head.py:181-240,305-354",
                 "point_sample.py:32-88", "baseline_r50_psg.py:351-389", "baseline.py:588-653"):
        assert cite in header, cite


def test_bad_arguments_are_refused_without_launching(built_lib):
    from pairnet_amd import hip
    lib = hip.lib()
    N = None
    assert lib.pn_uniform_f32(N, 4, 1, 0, 0, 0, 0, 0, N) == -1
    assert lib.pn_uniform_f32(1 << 20, 0, 1, 0, 0, 0, 0, 0, N) == -1
    assert lib.pn_seg_targets(N, N, N, N, 0, N, 0, 0, 2, 2, 8, 5, 0, N, N, N, N, N) == -1
    assert lib.pn_uncertain_points_f32(N, 1, N, 1, 1, 1, 4, 4, N, N, 6, 2, 3, N, N, N) == -1
    assert lib.pn_uncertain_points_f32(1 << 20, 1, 1 << 20, 1, 1, 1, 4, 4, 1 << 20, 1 << 20, 6, 4, 3,
                                       1 << 20, 1 << 20, N) == -1          # k > Np
    assert lib.pn_point_sample_rows_f32(N, 0, 1, N, N, N, 1, 4, 4, 3, N) == -1
    assert lib.pn_point_sample_rows_f32(1 << 20, 0, 1, 1 << 20, 1 << 20, 1 << 20, 70000, 4, 4, 3, N) == -1
    assert lib.pn_mask_point_loss_f32(N, N, N, 4, 3, 2, 2, 1.0, 1.0, 1.0, 0.0, N, N, N, N) == -1
    assert lib.pn_mask_point_loss_f32(1 << 20, 1 << 20, 1 << 20, 5, 3, 2, 2, 1.0, 1.0, 1.0, 0.0, 1 << 20,
                                      1 << 20, N, N) == -1                 # M != L * Ml
    assert lib.pn_point_scatter_grad_f32(N, N, N, N, 1, 3, 4, 4, N) == -1
    assert lib.pn_point_scatter_scratch_ints(2, 50, 13, 21) == 2 * (14 * 22 + 100)
    assert lib.pn_ce_avg_f32(N, N, N, N, 1, 8, 6, 1.0, N) == -1
    assert lib.pn_ce_avg_f32(1 << 20, 1 << 20, 1 << 20, 1 << 20, 1, 4097, 6, 1.0, N) == -1
    assert lib.pn_ce_avg_grad_f32(1 << 20, 1 << 20, N, 1 << 20, 1, 8, 6, 1.0, N) == -1


def test_option_sets_outside_the_config_are_refused():
    from pairnet_amd.seg_losses import Mask2FormerLoss
    Mask2FormerLoss(5, 8)
    for kw in (dict(loss_cls=dict(type="FocalLoss")), dict(loss_mask=dict(type="CrossEntropyLoss")),
               dict(loss_dice=dict(type="DiceLoss", use_sigmoid=True, activate=True, naive_dice=False)),
               dict(train_cfg=dict(mask_assigner=dict(
                   type="MaskHungarianAssigner", cls_cost=dict(type="FocalLossCost", weight=1.0),
                   mask_cost=dict(type="CrossEntropyLossCost", weight=5.0, use_sigmoid=True),
                   dice_cost=dict(type="DiceCost", weight=5.0, pred_act=True, eps=1.0))))):
        with pytest.raises(NotImplementedError):
            Mask2FormerLoss(5, 8, **kw)


def test_seg_loss_kernels_compile_for_gfx950_without_scratch(tmp_path):
    from pairnet_amd import build as B
    out = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(B.CSRC, "seg_loss.hip"), "-o", str(tmp_path / "seg_loss.o")],
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
    names = ("k_uniform", "k_seg_targets", "k_uncertain_points", "k_point_sample_rows",
             "k_mask_point_sums", "k_mask_point_finish", "k_mask_point_coef", "k_point_scatter_grad",
             "k_ce_avg", "k_ce_avg_grad")
    for n in names:
        hit = [k for k in res if n in k]
        assert hit, (n, sorted(res))
        for k in hit:
            assert res[k]["ScratchSize [bytes/lane]"] == 0, k
            assert res[k]["LDS Size [bytes/block]"] <= 17 * 1024, k
