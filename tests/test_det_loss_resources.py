"""CPU: register, LDS and scratch figures of the detection-loss kernels (csrc/det_loss.hip) from a
gfx950 cross-compile with the library's own flags (-Rpass-analysis=kernel-resource-usage), the way
tests/test_grouped_conv_resources.py reads them.

k_det_focal is the streaming kernel (13 M elements at the config's shapes): it must not spill, and
its LDS (one slot per lane and term, DET_MAX_TERMS = 16: 16 KiB + the wave sums) must leave room for
several workgroups per CU."""
from test_fused_passes_resources import _usage

KERNELS = ("k_det_match_cost", "k_det_focal", "k_det_focal_final", "k_det_box_loss", "k_det_results")


def test_det_loss_kernels_have_no_scratch(tmp_path):
    res = _usage("det_loss.hip", tmp_path)
    found = {}
    for want in KERNELS:
        hits = [k for k in res if want in k and (want != "k_det_focal" or "final" not in k)]
        assert len(hits) == 1, (want, sorted(res))
        found[want] = res[hits[0]]
    for name, u in found.items():
        print("%-20s VGPRs %3d AGPRs %3d waves/SIMD %d LDS %6d B scratch %d B/lane" % (
            name, u["VGPRs"], u["AGPRs"], u["Occupancy [waves/SIMD]"], u["LDS Size [bytes/block]"],
            u["ScratchSize [bytes/lane]"]))
        assert u["ScratchSize [bytes/lane]"] == 0, name
    focal = found["k_det_focal"]
    assert focal["LDS Size [bytes/block]"] <= 32 * 1024
    assert focal["Occupancy [waves/SIMD]"] >= 4
