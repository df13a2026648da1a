"""GPU: the encoder's FFN as one launch (csrc/gemm_s3.hip, k_gemm_s3_ffn / pn_gemm_s3_ffn_f32).

The launch must be the two pn_gemm_s3_f32 calls it replaces -- FFN-1 with ReLU written as an S3
operand, FFN-2 with the S3 residual and the LayerNorm -- bit for bit, in every output form (fp32
rows, S3 of out, S3 of out + pos), padding rows of the S3 buffers included: the same products in
the same order, only the hidden rows never reach memory.

Shapes: M = 96 (one tile), 100 (a ragged 32-row block), 131 (a ragged 96-row tile), 288 (three
tiles); F = 256, 512, 1024 (one, two, four hidden chunks); K = N = 256."""
import ctypes

import pytest
import torch
import torch.nn.functional as F_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MS, FS = (96, 100, 131, 288), (256, 512, 1024)


@pytest.fixture(scope="module")
def hip(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip as h
    h.lib()
    return h


def s3(hip, x):
    out = torch.zeros(hip.s3_floats(x.shape[0], x.shape[1]), device=DEV)
    hip.s3_split(x, out)
    return out


def joined(hip, s, rows, K):
    out = torch.full((rows, K), float("nan"), device=DEV)
    hip.s3_join(s, out)
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def operands(hip, M, F, integer=False):
    """x [M x 256], W1 [F x 256], b1, W2 [256 x F], b2, res [M x 256], pos (fewer rows than M),
    gamma, beta.  integer: small integers sized so that every partial sum is exact in fp32 --
    |hidden| <= 4 * 2 * 256 + 8 < 2^12, |sum| <= 2^12 * 1024 + 8 + 4 < 2^23 -- and gamma = 1,
    beta = 0."""
    g = torch.Generator().manual_seed(1000 * M + F + (7 if integer else 0))
    if integer:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float().to(DEV)
        x, w1, b1 = ri(-4, 4, M, 256), ri(-2, 2, F, 256), ri(-8, 8, F)
        w2, b2, res = ri(-1, 1, 256, F), ri(-8, 8, 256), ri(-4, 4, M, 256)
        gamma, beta = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)
    else:
        rn = lambda scale, *s: (torch.randn(*s, generator=g) * scale).to(DEV)
        x, w1, b1 = rn(1.0, M, 256), rn(1 / 16, F, 256), rn(1.0, F)
        w2, b2, res = rn(1 / 16, 256, F), rn(1.0, 256), rn(1.0, M, 256)
        gamma, beta = rn(0.2, 256) + 1.0, rn(1.0, 256)
    pos = (torch.randn(max(1, M // 3), 256, generator=g)).to(DEV)
    if integer:
        pos = pos.round()
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, res=res, pos=pos, gamma=gamma, beta=beta)


def outputs(hip, M):
    return dict(out=torch.full((M, 256), float("nan"), device=DEV),
                out_s3=torch.zeros(hip.s3_floats(M, 256), device=DEV),
                out_s3_pos=torch.zeros(hip.s3_floats(M, 256), device=DEV))


def two_launches(hip, o, M, F):
    """The reference: hip.gemm_s3 twice on the same S3 buffers; returns (outputs, hidden S3)."""
    xs, w1s, w2s, rs = s3(hip, o["x"]), s3(hip, o["w1"]), s3(hip, o["w2"]), s3(hip, o["res"])
    hs = torch.zeros(hip.s3_floats(M, F), device=DEV)
    hip.gemm_s3(xs, w1s, M, F, 256, bias=o["b1"], relu=True, out_s3=hs)
    ref = outputs(hip, M)
    hip.gemm_s3(hs, w2s, M, 256, F, bias=o["b2"], res_s3=rs, gamma=o["gamma"], beta=o["beta"],
                pos=(hip.pos8(o["pos"]), o["pos"].shape[0]), **ref)
    return ref, hs, (xs, w1s, w2s, rs)


def one_launch(hip, o, M, F, bufs):
    xs, w1s, w2s, rs = bufs
    got = outputs(hip, M)
    hip.gemm_s3_ffn(xs, w1s, w2s, M, 256, 256, F, b1=o["b1"], b2=o["b2"], res_s3=rs,
                    gamma=o["gamma"], beta=o["beta"], pos=(hip.pos8(o["pos"]), o["pos"].shape[0]),
                    **got)
    return got


_CASES = {}


def case(hip, M, F, integer=False):
    """Operands, the two-launch reference and the one-launch result of a shape, computed once."""
    key = (M, F, integer)
    if key not in _CASES:
        o = operands(hip, M, F, integer)
        ref, hs, bufs = two_launches(hip, o, M, F)
        got = one_launch(hip, o, M, F, bufs)
        torch.cuda.synchronize()
        _CASES[key] = (o, ref, hs, bufs, got)
    return _CASES[key]


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("M", MS)
def test_one_launch_is_the_two_launches_bit_for_bit(hip, M, F):
    _, ref, _, _, got = case(hip, M, F)
    assert torch.isfinite(ref["out"]).all()
    for k in ("out", "out_s3", "out_s3_pos"):
        assert torch.equal(bits(got[k]), bits(ref[k])), (k, M, F)
    # (the forms agree with each other: the S3 outputs hold out and out + pos[row % len])
    o = _CASES[(M, F, False)][0]
    assert torch.equal(joined(hip, got["out_s3"], M, 256), got["out"])
    want_p = got["out"] + o["pos"][torch.arange(M, device=DEV) % o["pos"].shape[0]]
    assert torch.equal(joined(hip, got["out_s3_pos"], M, 256), want_p)


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("M", MS)
def test_integer_problems_are_exact(hip, M, F):
    """Small-integer operands, gamma = 1, beta = 0: the hidden rows and the sums in front of the
    LayerNorm are integers below 2^24, so the two-launch form holds them exactly (checked: its
    hidden rows, and its FFN-2 without the LayerNorm, equal the fp64 integer result), and the one
    launch equals the two-launch form bit for bit under the same operands -- the LayerNorm of equal
    sums.  Against torch's fp64 LayerNorm of the integer sums: 2e-5 of the output scale, the bar of
    the LayerNorm row epilogue's own test (tests/test_gemm_s3_gpu.py)."""
    o, ref, hs, bufs, got = case(hip, M, F, integer=True)
    hidden = (o["x"].double() @ o["w1"].double().T + o["b1"].double()).clamp_min(0)
    assert hidden.abs().max() < 2 ** 12
    assert torch.equal(joined(hip, hs, M, F).double(), hidden)
    z = hidden @ o["w2"].double().T + o["b2"].double()
    assert (z.abs().max() + 4) < 2 ** 23
    plain = torch.full((M, 256), float("nan"), device=DEV)
    hip.gemm_s3(hs, bufs[2], M, 256, F, bias=o["b2"], out=plain)
    assert torch.equal(plain.double(), z)
    for k in ("out", "out_s3", "out_s3_pos"):
        assert torch.equal(bits(got[k]), bits(ref[k])), (k, M, F)
    want = F_.layer_norm(z + o["res"].double(), (256,), None, None, 1e-5)
    assert (got["out"].double() - want).abs().max() <= 2e-5 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("M,F", [(131, 1024), (288, 512)])
def test_two_launches_of_the_kernel_give_equal_bits(hip, M, F):
    o, _, _, bufs, got = case(hip, M, F)
    again = one_launch(hip, o, M, F, bufs)
    for k in ("out", "out_s3", "out_s3_pos"):
        assert torch.equal(bits(again[k]), bits(got[k])), k


def test_unhandled_shapes_and_activations_are_refused_without_launching(hip):
    M, F = 96, 256
    o, _, _, (xs, w1s, w2s, rs), _ = case(hip, M, F)
    out = torch.full((M, 256), 3.0, device=DEV)
    kw = dict(b1=o["b1"], b2=o["b2"], res_s3=rs, gamma=o["gamma"], beta=o["beta"], out=out)
    with pytest.raises(RuntimeError):
        hip.gemm_s3_ffn(xs, w1s, w2s, M, 256, 128, F, **kw)            # K = 128
    with pytest.raises(RuntimeError):
        hip.gemm_s3_ffn(xs, w1s, w2s, M, 128, 256, F, **kw)            # N = 128
    with pytest.raises(RuntimeError):
        hip.gemm_s3_ffn(xs, w1s, w2s, M, 256, 256, 384, **kw)          # F = 384
    with pytest.raises(RuntimeError):
        hip.gemm_s3_ffn(xs, w1s, w2s, M, 256, 256, F, gelu=True, **kw)
    with pytest.raises(RuntimeError):                                  # no LayerNorm
        hip.gemm_s3_ffn(xs, w1s, w2s, M, 256, 256, F, b1=o["b1"], b2=o["b2"], res_s3=rs, out=out)
    d = hip.GemmS3FfnDesc()                                            # all NULL
    assert hip.lib().pn_gemm_s3_ffn_f32(ctypes.byref(d), None) == -1
    torch.cuda.synchronize()
    assert torch.all(out == 3.0)                                       # nothing ran


def test_head_encoder_memory_is_the_same_bits_with_and_without_the_fusion():
    """The 96 x 128 head fixture: pl.X (the encoder's memory) and the head's outputs with
    fuse_encoder_ffn 0 and 1; the switch is part of the stage graphs' configuration."""
    from helpers import head_cfg, oracle_head
    from pairnet_amd import CrossHead2
    _, sd, _ = oracle_head(1234)
    head = CrossHead2(**head_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    assert head.gemm_arithmetic == "bf16x3" and head.enc_ffn % 256 == 0
    H, W = 96, 128
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(1, c, H // s, W // s, generator=g).to(DEV)
             for c, s in zip((256, 512, 1024, 2048), (4, 8, 16, 32))]
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4)]
    seen = {}
    for fuse in (0, 1):
        head.fuse_encoder_ffn = fuse
        cls, mask = head.forward(feats, metas)
        torch.cuda.synchronize()
        pl = head._last_plan
        seen[fuse] = (pl.X.clone(), pl.graph_cfg, cls["rel"].clone(), mask["mask"].clone())
    assert seen[0][1] != seen[1][1]
    assert torch.isfinite(seen[1][0]).all()
    for a, b in zip(seen[0][::2] + seen[0][3:], seen[1][::2] + seen[1][3:]):
        assert torch.equal(bits(a), bits(b))
