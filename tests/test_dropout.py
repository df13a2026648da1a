"""CPU: the counter-based dropout of the relation decoder's FFN (csrc/dropout.hip) -- the numpy
reference of its mask against the algorithm's published known answers and pinned dropped counts,
the kernels' register / scratch figures from a gfx950 cross-compile, header <-> binding, and the
trainer's refusal of dropout rates it cannot honour."""
import os
import re
import subprocess

import numpy as np
import pytest

import dropout_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_reference_reproduces_the_published_known_answers(ctr, key, want):
    assert _hex(ref.philox4x32_10(ctr, key)) == want


@pytest.mark.parametrize("p,n,seed,subseq,step,site,dropped", [
    (0.1, 204800, 0, 0, 0, 0, 20304),
    (0.1, 25600, 0, 0, 0, 1, 2542),
    (0.1, 204800, 0, 1, 0, 0, 20409),
    (0.1, 204800, 0x0123456789abcdef, 0, 7, 11, 20543),
    (0.5, 204800, 0, 0, 0, 0, 102164),
])
def test_reference_dropped_counts_under_the_counter_layout(p, n, seed, subseq, step, site, dropped):
    keep = ref.keep_mask(n, p, seed, subseq, step, site)
    assert keep.dtype == np.uint8 and keep.shape == (n,)
    got = int(n - keep.sum())
    pf = float(np.float32(p))
    assert abs(got - n * pf) < 4 * np.sqrt(n * pf * (1 - pf))
    assert got == dropped


def test_reference_threshold_scale_and_first_bits():
    assert ref.threshold(0.1) == 429496736 and ref.threshold(0.0) == 0
    assert ref.scale(0.0) == np.float32(1.0)
    assert ref.scale(0.1) == np.float32(1.0 / (1.0 - float(np.float32(0.1))))
    keep = ref.keep_mask(16, 0.1, 0, 0, 0, 0)
    assert "".join(str(int(b)) for b in keep) == "1111111001111111"
    # a prefix of a longer mask is the shorter mask (the element index alone addresses a bit)
    assert np.array_equal(ref.keep_mask(1023, 0.5, 3, 1, 2, 5), ref.keep_mask(4096, 0.5, 3, 1, 2, 5)[:1023])


def test_dropout_kernels_fit_in_registers_without_scratch(tmp_path):
    """Ten Philox rounds on four words plus a float4 or two: 0 bytes of scratch, no AGPRs, at most
    64 VGPRs (occupancy 8 waves / SIMD), under the library's own flags."""
    from pairnet_amd import build as B
    assert "dropout" in B.SOURCES
    out = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(B.CSRC, "dropout.hip"), "-o", str(tmp_path / "dropout.o")],
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
    kernels = {k: v for k, v in res.items() if "k_dropout" in k}
    # pn_dropout_f32 without / with the residual operand, pn_dropout_keep_u8
    assert len(kernels) == 3 and sum("k_dropout_keep" in k for k in kernels) == 1, sorted(res)
    for k, u in kernels.items():
        print(k, u)
        assert u["ScratchSize [bytes/lane]"] == 0, k
        assert u["AGPRs"] == 0 and u["VGPRs"] <= 64, k
        assert u["Occupancy [waves/SIMD]"] >= 8, k


def test_header_and_binding_declare_the_two_entries():
    from pairnet_amd import hip
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    declared = set(re.findall(r"\b(pn_[a-z0-9_]+)\s*\(", header))
    for name in ("pn_dropout_f32", "pn_dropout_keep_u8"):
        assert name in declared and name in hip._SIGS and name in hip.EXPORTS, name
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION
    assert len(hip._SIGS["pn_dropout_f32"][1]) == 10 and len(hip._SIGS["pn_dropout_keep_u8"][1]) == 8
    assert callable(hip.dropout) and callable(hip.dropout_keep)


def test_bad_arguments_are_refused_without_a_gpu(built_lib):
    """The argument checks run before any launch: they need no device (pointers are only tested
    for NULL and alignment)."""
    from pairnet_amd import hip
    lib = hip.lib()
    ok = 4096                                                 # a 16-byte aligned non-NULL "pointer"
    assert lib.pn_dropout_f32(None, None, ok, 16, 0.1, 0, 0, 0, 0, None) == -1
    assert lib.pn_dropout_f32(ok, None, None, 16, 0.1, 0, 0, 0, 0, None) == -1
    assert lib.pn_dropout_f32(ok, None, ok, 0, 0.1, 0, 0, 0, 0, None) == -1
    assert lib.pn_dropout_f32(ok, None, ok, (1 << 34) + 1, 0.1, 0, 0, 0, 0, None) == -1
    for p in (1.0, -0.1, 1.5, float("nan")):
        assert lib.pn_dropout_f32(ok, None, ok, 16, p, 0, 0, 0, 0, None) == -1
        assert lib.pn_dropout_keep_u8(ok, 16, p, 0, 0, 0, 0, None) == -1
    assert lib.pn_dropout_f32(ok + 4, None, ok, 16, 0.1, 0, 0, 0, 0, None) == -1
    assert lib.pn_dropout_f32(ok, ok + 8, ok, 16, 0.1, 0, 0, 0, 0, None) == -1
    assert lib.pn_dropout_f32(ok, None, ok + 4, 16, 0.1, 0, 0, 0, 0, None) == -1
    assert lib.pn_dropout_keep_u8(None, 16, 0.1, 0, 0, 0, 0, None) == -1
    assert lib.pn_dropout_keep_u8(ok, 0, 0.1, 0, 0, 0, 0, None) == -1
    assert lib.pn_dropout_keep_u8(ok, (1 << 34) + 1, 0.1, 0, 0, 0, 0, None) == -1


def test_head_records_the_configured_rates_and_the_trainer_refuses_what_it_cannot_honour():
    """`helpers.head_cfg()` carries the reference's ffn_drop=0.1 for the relation decoder and 0.0
    elsewhere.  `dropout=True` on a config with any other non-zero rate is refused by name; the
    check runs before anything touches a device."""
    from helpers import head_cfg
    from pairnet_amd import CrossHead2, TailTrainer
    from pairnet_amd.grad import FfnDropout
    head = CrossHead2(**head_cfg())
    assert head.rel_ffn_drop == 0.1 and head.other_drop_rates == {}
    assert TailTrainer._dropout_rate(head, True) == 0.1
    assert TailTrainer._dropout_rate(head, False) == 0.0
    assert TailTrainer._dropout_rate(head, 0.25) == 0.25
    with pytest.raises(ValueError):
        TailTrainer._dropout_rate(head, 1.0)
    for path, key in ((("transformer_decoder", "transformerlayers", "ffn_cfgs"), "ffn_drop"),
                      (("transformer_decoder", "transformerlayers", "attn_cfgs"), "attn_drop"),
                      (("relation_decoder", "transformerlayers", "attn_cfgs"), "proj_drop"),
                      (("pixel_decoder", "encoder", "transformerlayers", "attn_cfgs"), "dropout"),
                      (("pixel_decoder", "encoder", "transformerlayers", "ffn_cfgs"), "ffn_drop")):
        cfg = head_cfg()
        node = cfg
        for k in path:
            node = node[k]
        node[key] = 0.1
        bad = CrossHead2(**cfg)
        dotted = ".".join(path + (key,))
        assert bad.other_drop_rates == {dotted: 0.1}
        with pytest.raises(NotImplementedError, match=re.escape(dotted)):
            TailTrainer(bad, dropout=True)
        assert TailTrainer._dropout_rate(bad, 0.1) == 0.1     # an explicit rate is the caller's call
    cfg = head_cfg()
    cfg["transformer_decoder"]["transformerlayers"]["ffn_cfgs"]["dropout_layer"] = dict(
        type="DropPath", drop_prob=0.2)
    with pytest.raises(NotImplementedError, match="dropout_layer"):
        TailTrainer(CrossHead2(**cfg), dropout=True)
    # the descriptor: sites 2 * layer + {0, 1}, rates outside [0, 1) refused
    d = FfnDropout(0.1, seed=5, subseq=1, step=7)._replace(layer=3)
    assert (d.p, d.seed, d.subseq, d.step, d.layer) == (0.1, 5, 1, 7, 3)
    with pytest.raises(ValueError):
        FfnDropout(1.0)
