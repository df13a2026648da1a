"""CPU: the deterministic deformable-attention backward (`pn_msda_bwd_det_f32`,
csrc/msda_grad.hip) is declared, bound and built; refuses bad arguments without a device; sizes its
scratch; compiles for gfx950 without spilling; the order case of tests/msda_det_ref.py can tell
summation orders apart; the `deterministic` keywords exist with their defaults.  The kernels
themselves run in tests/test_msda_det_gpu.py and tests/test_deterministic_train_gpu.py."""
import inspect
import os
import re
import subprocess

import numpy as np

import msda_det_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pn_msda_bwd_det_scratch_bytes", "pn_msda_bwd_det_f32")


def test_header_binding_and_build_declare_the_entries():
    from pairnet_amd import build as B
    from pairnet_amd import hip
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    for name in ENTRIES:
        assert name in declared and name in hip._SIGS and name in hip.EXPORTS, name
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION == 34
    assert "msda_grad" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "msda_grad.hip"))
    for cite in ("mmcv/ops/csrc/pytorch/cuda/ms_deform_attn_cuda.cu", "ms_deformable_col2im",
                 "((q*L + l)*4 + p)*4 + t", "ASCENDING id"):
        assert cite in header, cite
    assert callable(hip.msda_bwd_det) and callable(hip.msda_bwd_det_scratch_bytes)
    assert len(hip._SIGS["pn_msda_bwd_det_f32"][1]) == 17


def test_scratch_size_is_bounded_and_zero_for_bad_arguments(built_lib):
    from pairnet_amd import hip
    for args in ((2, 21950, 21950, 3), (1, 12, 1, 1)):
        need, low = hip.msda_bwd_det_scratch_bytes(*args), R.scratch_lower_bound(*args)
        print(args, need, low)
        assert low <= need <= 1.25 * low, (args, need, low)
    for bad in ((0, 12, 1, 1), (1, 0, 1, 1), (1, 12, 0, 1), (1, 12, 1, 0), (1, 12, 1, 5),
                (-1, 12, 1, 1), (1, 12, 1 << 27, 1), (2, 12, 1 << 23, 1), (1, 12, 1 << 25, 4)):
        assert hip.msda_bwd_det_scratch_bytes(*bad) == 0, bad


def test_bad_arguments_are_refused_without_launching(built_lib):
    """Nothing here reaches a launch: no device is needed (the pointers are made-up addresses)."""
    from pairnet_amd import hip
    lib = hip.lib()
    P, BIG = 0x10000, 1 << 40                 # a 16-byte aligned non-NULL address; plenty of scratch
    B, N, Nq, L = 1, 12, 3, 1
    need = hip.msda_bwd_det_scratch_bytes(B, N, Nq, L)
    assert need > 0

    def call(ptrs=None, ld=256, scratch=P, nbytes=BIG, dims=(B, N, Nq, L)):
        ptrs = [P] * 9 if ptrs is None else ptrs
        return lib.pn_msda_bwd_det_f32(ptrs[0], ld, *ptrs[1:], scratch, nbytes, *dims, None)

    # everything pn_msda_bwd_f32 refuses
    assert lib.pn_msda_bwd_f32(P, 256, *([P] * 8), 0, N, Nq, L, None) == -1
    for i in range(9):                                                   # a NULL operand
        assert call([None if j == i else P for j in range(9)]) == -1, i
    for dims in ((0, N, Nq, L), (B, 0, Nq, L), (B, N, 0, L), (B, N, Nq, 0), (B, N, Nq, 5)):
        assert call(dims=dims) == -1, dims
    for ld in (255, 128, 258):
        assert call(ld=ld) == -1, ld
    for i, off in ((0, 8), (6, 8), (5, 8), (3, 4), (7, 4)):   # value, grad_value, grad_output: 16 B;
        ptrs = [P] * 9                                         # locations, grad_sampling_loc: 8 B
        ptrs[i] = P + off
        assert call(ptrs) == -1, i
    # the scratch
    assert call(scratch=None) == -1
    assert call(nbytes=need - 1) == -1
    assert call(nbytes=0) == -1
    assert call(scratch=P + 8) == -1
    # record ids / slots past int32
    assert call(dims=(1, N, 1 << 27, 1)) == -1
    assert call(dims=(1, N, 1 << 25, 4)) == -1
    assert call(dims=(2, N, 1 << 23, 1)) == -1


def test_kernels_compile_for_gfx950_without_scratch(tmp_path):
    from pairnet_amd import build as B
    out = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(B.CSRC, "msda_grad.hip"), "-o", str(tmp_path / "msda_grad.o")],
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
    for stem in ("k_msda_bwd_count", "k_msda_bwd_fill", "k_msda_bwd_sum", "k_scan_block_sums",
                 "k_scan_top", "k_scan_finish"):
        assert any(stem in k for k in res), (stem, sorted(res))
    assert len(res) >= 15                       # count / fill / sum for L = 1..4, three scan kernels
    for k, use in res.items():
        print(k, use)
        assert use["ScratchSize [bytes/lane]"] == 0, k
        assert use["LDS Size [bytes/block]"] <= 64 * 1024, k


def test_the_order_case_tells_summation_orders_apart():
    case = R.order_case(0)
    con, gout = case["contributions"], case["gout"].numpy()
    planted = case["planted"]
    assert len(planted) >= 8
    assert max(len(v) for v in con.values()) > 32          # more than a half-wave of records
    once_equal = 0
    for b, tok, head in planted:
        recs = con[(b, tok, head)]
        assert [r[0] for r in recs] == sorted(r[0] for r in recs)
        want = case["expected"][b, tok, head].numpy()
        assert np.array_equal(want, R.ordered_sum(recs, gout[b], head))
        n = len(recs)
        down = R.ordered_sum(recs, gout[b], head, order=range(n - 1, -1, -1))
        evens = [i for i in range(n) if recs[i][0] % 2 == 0]
        odds = [i for i in range(n) if recs[i][0] % 2 == 1]
        even_odd = R.ordered_sum(recs, gout[b], head, order=evens + odds)
        assert (down != want).any(), (b, tok, head)
        assert (even_odd != want).any(), (b, tok, head)
        g = gout[b][[r[2] for r in recs]][:, head * 32:(head + 1) * 32].astype(np.float64)
        exact = (np.array([r[1] for r in recs], np.float64)[:, None] * g).sum(0)   # exact in fp64
        once_equal += bool(np.array_equal(exact.astype(np.float32), want))
    # not order-independent by accident: the sequential sum is not simply the exact sum rounded
    assert once_equal < len(planted), once_equal
    # every product is exact: coef x g has at most a handful of significant bits
    for recs in con.values():
        for _, coef, _ in recs:
            assert coef == 0 or float(np.log2(coef)).is_integer()


def test_deterministic_keywords_and_defaults():
    from pairnet_amd.baseline_head import CrossHeadBaseline
    from pairnet_amd.baseline_train import BaselineTrainer
    from pairnet_amd.grad import PixelDecoderGrad
    from pairnet_amd.mmcv_ops import ms_deform_attn_backward
    from pairnet_amd.seg_grad import SegPixelDecoderGrad
    from pairnet_amd.train import TailTrainer
    for fn, default in ((TailTrainer.__init__, False), (BaselineTrainer.__init__, False),
                        (ms_deform_attn_backward, None),
                        (CrossHeadBaseline.segmenter_backward, False),
                        (CrossHeadBaseline.full_backward, False)):
        par = inspect.signature(fn).parameters
        assert "deterministic" in par, fn
        assert par["deterministic"].default is default, fn
    assert PixelDecoderGrad.deterministic is False and SegPixelDecoderGrad.deterministic is False
    assert PixelDecoderGrad.msda_scratch is None
