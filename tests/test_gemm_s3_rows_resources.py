"""CPU: register / LDS / scratch figures of the row-reading LayerNorm GEMM (csrc/gemm_s3.hip,
k_gemm_s3_rows) from a gfx950 cross-compile with the library's own flags
(-Rpass-analysis=kernel-resource-usage), by the method of tests/test_gemm_s3_ffn_resources.py.

The kernel runs as ONE workgroup of 8 waves per CU (two waves per SIMD), so a wave has at most 256
registers, vector and accumulation together: a stage's fragments (96), the accumulators (48), the
8 held row values and the 12 piece registers of the half stage it forms, without spilling."""
import pytest

from test_gemm_s3_ffn_resources import _one, _usage


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("gemm_s3.hip", tmp_path_factory.mktemp("usage_rows"))


def test_rows_kernel_fits_one_workgroup_per_cu_without_scratch(usage):
    u = _one(usage, "k_gemm_s3_rows")
    print("k_gemm_s3_rows", u)
    assert u["ScratchSize [bytes/lane]"] == 0
    assert u["LDS Size [bytes/block]"] <= 160 * 1024
    # 8 waves per CU are 2 per SIMD, 512 / 2 registers each
    assert u["VGPRs"] + u["AGPRs"] <= 256
    assert u["Occupancy [waves/SIMD]"] >= 2


def test_dual_split_kernel_has_no_scratch(usage):
    u = _one(usage, "k_s3_split2")
    print("k_s3_split2", u)
    assert u["ScratchSize [bytes/lane]"] == 0 and u["LDS Size [bytes/block]"] == 0
