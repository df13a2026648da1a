"""CPU: register / LDS / scratch figures of the one-launch encoder FFN (csrc/gemm_s3.hip,
k_gemm_s3_ffn) and of the kernels it shares the file with, from a gfx950 cross-compile with the
library's own flags (-Rpass-analysis=kernel-resource-usage).

The kernel runs as ONE workgroup of 8 waves per CU (two waves per SIMD), so a wave has at most 256
registers, vector and accumulation together; it holds two accumulator sets, a stage's fragments
and its 18 KiB piece of the hidden rows at once and must do so without spilling.  The other
k_gemm_s3* kernels' figures are those measured before it was added: sharing the LayerNorm row
epilogue with it must not change them."""
import os
import re
import subprocess

import pytest

from pairnet_amd import build as B


def _usage(src, tmp_path):
    out = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(B.CSRC, src), "-o", str(tmp_path / (src + ".o"))],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+(.*)", line)
        if not m:
            continue
        t = m.group(1)
        f = re.match(r"Function Name: (\S+)", t)
        if f:
            cur = res.setdefault(f.group(1), {})
            continue
        kv = re.match(r"(.+?): (\d+)", t)
        if kv and cur is not None:
            cur[kv.group(1).strip()] = int(kv.group(2))
    return res


def _one(res, needle):
    hits = [k for k in res if needle in k]
    assert len(hits) == 1, (needle, hits)
    return res[hits[0]]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("gemm_s3.hip", tmp_path_factory.mktemp("usage"))


def test_ffn_kernel_fits_one_workgroup_per_cu_without_scratch(usage):
    u = _one(usage, "k_gemm_s3_ffn")
    print("k_gemm_s3_ffn", u)
    assert u["ScratchSize [bytes/lane]"] == 0
    assert u["LDS Size [bytes/block]"] <= 160 * 1024
    assert u["VGPRs"] + u["AGPRs"] <= 512
    # what the launch needs: 8 waves per CU are 2 per SIMD, 512 / 2 registers each
    assert u["VGPRs"] + u["AGPRs"] <= 256 and u["Occupancy [waves/SIMD]"] >= 2


@pytest.mark.parametrize("kernel,vgprs,agprs,lds", [
    ("k_gemm_s3ILb0EE", 158, 0, 153600),
    ("k_gemm_s3ILb1EE", 160, 0, 153600),       # shares s3_ln_epilogue with the FFN kernel
    ("k_gemm_s3_wide", 162, 0, 110592),
    ("k_gemm_s3_narrow", 110, 16, 0),
])
def test_other_split_gemm_kernels_are_unchanged(usage, kernel, vgprs, agprs, lds):
    u = _one(usage, kernel)
    print(kernel, u)
    assert u["ScratchSize [bytes/lane]"] == 0
    assert (u["VGPRs"], u["AGPRs"], u["LDS Size [bytes/block]"]) == (vgprs, agprs, lds)
    assert u["Occupancy [waves/SIMD]"] >= 2
