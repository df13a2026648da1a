"""CPU: register / scratch / occupancy figures of the kernels that absorbed a neighbouring pass,
and of the default tile GEMM they share a loop with, from a gfx950 cross-compile with the
library's own flags (-Rpass-analysis=kernel-resource-usage).

The persistent tile kernels are launched with as many workgroups per CU as their registers allow
(5 for the 64x64 instantiations: 96 VGPRs); a new mode of the shared loop must neither push the
default instantiation over that bound nor spill itself."""
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
def gemm_usage(tmp_path_factory):
    return _usage("gemm.hip", tmp_path_factory.mktemp("usage"))


@pytest.mark.parametrize("kernel,max_vgprs,min_waves", [
    ("k_gemm_tileILi64ELi64ELi32ELi32ELi0ELb0EE", 96, 5),     # the default instantiation: unchanged
    ("k_gemm_tileILi64ELi64ELi32ELi32ELi2ELb0EE", 96, 5),     # implicit-GEMM convolution
    ("k_gemm_stencil5GemmP", 96, 5),
    ("k_gemm_stencil_gather", 96, 5),                          # + make_tap row addresses per tile
    ("k_gemm_proj", 96, 5),                                    # + 16 kept shortcut values per lane
])
def test_tile_gemm_modes_fit_five_workgroups_without_scratch(gemm_usage, kernel, max_vgprs, min_waves):
    u = _one(gemm_usage, kernel)
    print(kernel, u)
    assert u["ScratchSize [bytes/lane]"] == 0
    assert u["VGPRs"] <= max_vgprs and u["AGPRs"] == 0
    assert u["Occupancy [waves/SIMD]"] >= min_waves
    assert u["LDS Size [bytes/block]"] * 5 <= 160 * 1024


def test_groupnorm_upadd_fits_its_sixteen_waves(tmp_path):
    u = _one(_usage("norm.hip", tmp_path), "k_gn_apply_up")
    print(u)
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] <= 128
    assert u["Occupancy [waves/SIMD]"] >= 4      # one 1024-thread workgroup per CU
