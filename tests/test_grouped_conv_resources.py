"""CPU: scratch, LDS and register figures of the grouped-convolution kernels
(csrc/grouped_conv.hip) from a gfx950 cross-compile with the library's own flags
(-Rpass-analysis=kernel-resource-usage), the way tests/test_fused_passes_resources.py reads them.

The kernels keep a 16-channel tile's weights in registers (9 max(Cg, 16) / 4 per lane: 36 .. 144)
and the halo patch in LDS; a spill would put the weights in scratch memory inside the MFMA loop."""
from test_fused_passes_resources import _usage


def test_grouped_conv_kernels_have_no_scratch_and_fit_lds(tmp_path):
    res = _usage("grouped_conv.hip", tmp_path)
    kernels = {k: v for k, v in res.items() if "k_conv3x3_grouped" in k}
    assert len(kernels) == 8, sorted(res)                 # Cg in {8, 16, 32, 64} x stride in {1, 2}
    for name, u in sorted(kernels.items()):
        print("%-60s VGPRs %3d AGPRs %3d waves/SIMD %d LDS %6d B" % (
            name, u["VGPRs"], u["AGPRs"], u["Occupancy [waves/SIMD]"], u["LDS Size [bytes/block]"]))
        assert u["ScratchSize [bytes/lane]"] == 0, name
        assert u["LDS Size [bytes/block]"] <= 160 * 1024, name
        assert u["Occupancy [waves/SIMD]"] >= 1
