"""GPU: the LayerNorm-row-epilogue GEMM that reads its activation operand as fp32 rows
(csrc/gemm_s3.hip, k_gemm_s3_rows / pn_gemm_s3_rows_ln_f32), and the two-output split
(k_s3_split2 / pn_s3_split2_f32).

The launch must be the pair it replaces -- hip.s3_split(A) -> hip.gemm_s3(res_s3=, gamma=, beta=) --
bit for bit in every output form (fp32 rows, S3 of out, S3 of out + pos), the padding rows of the S3
buffers included: the same pieces, the same products in the same order; only the split operand never
reaches memory.

Shapes: M = 1 (a single row), 33 (a ragged row block), 96 (one tile), 100 (a ragged block inside a
tile), 131 (a ragged tile), 288 (three tiles); K = 32, 64, 96 (one, two, three k-stages: the
prologue, the tail, every slot of the 3-slot A ring) and 256 (the production depth, the ring
re-used); row pitch K and K + 16.  In EVERY case A lives in an allocation of whole 96-row tiles
whose rows from M up and whose columns from K up are NaN: a loader that reads past M or past K
shows in the outputs (the reference's split wrote zeros into the padding rows) without anything
being provoked."""
import ctypes

import pytest
import torch
import torch.nn.functional as F_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MS, KS = (1, 33, 96, 100, 131, 288), (32, 64, 96, 256)
FORMS = ("out", "out_s3", "out_s3_pos")


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


def operands(M, K, pad, integer=False):
    """a: the [M x K] view (row pitch K + pad) of a NaN-filled allocation of whole 96-row tiles;
    w [256 x K], bias, res [M x 256], pos (fewer rows than M), gamma, beta.  integer: small integers,
    every partial sum exact in fp32 (|sum| <= 4 * 2 * 256 + 8 + 4 < 2^12), gamma = 1, beta = 0."""
    g = torch.Generator().manual_seed(1000 * M + K + pad + (7 if integer else 0))
    if integer:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float().to(DEV)
        x, w, bias, res = ri(-4, 4, M, K), ri(-2, 2, 256, K), ri(-8, 8, 256), ri(-4, 4, M, 256)
        gamma, beta = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)
    else:
        rn = lambda scale, *s: (torch.randn(*s, generator=g) * scale).to(DEV)
        x, w, bias, res = rn(1.0, M, K), rn(K ** -0.5, 256, K), rn(1.0, 256), rn(1.0, M, 256)
        gamma, beta = rn(0.2, 256) + 1.0, rn(1.0, 256)
    pos = torch.randn(max(1, M // 3), 256, generator=g).to(DEV)
    if integer:
        pos = pos.round()
    alloc = torch.full(((M + 95) // 96 * 96, K + pad), float("nan"), device=DEV)
    alloc[:M, :K] = x
    return dict(a=alloc[:M, :K], x=x, w=w, bias=bias, res=res, pos=pos, gamma=gamma, beta=beta)


def outputs(hip, M):
    return dict(out=torch.full((M, 256), float("nan"), device=DEV),
                out_s3=torch.zeros(hip.s3_floats(M, 256), device=DEV),
                out_s3_pos=torch.zeros(hip.s3_floats(M, 256), device=DEV))


def two_launches(hip, o, M, K):
    """The reference: hip.s3_split(A) -> hip.gemm_s3 with the row epilogue."""
    xs, ws, rs = s3(hip, o["a"]), s3(hip, o["w"]), s3(hip, o["res"])
    ref = outputs(hip, M)
    hip.gemm_s3(xs, ws, M, 256, K, bias=o["bias"], res_s3=rs, gamma=o["gamma"], beta=o["beta"],
                pos=(hip.pos8(o["pos"]), o["pos"].shape[0]), **ref)
    return ref, (xs, ws, rs)


def one_launch(hip, o, M, K, bufs):
    _, ws, rs = bufs
    got = outputs(hip, M)
    hip.gemm_s3_rows_ln(o["a"], ws, M, 256, K, bias=o["bias"], res_s3=rs, gamma=o["gamma"],
                        beta=o["beta"], pos=(hip.pos8(o["pos"]), o["pos"].shape[0]), **got)
    return got


_CASES = {}


def case(hip, M, K, pad=0, integer=False):
    """Operands, the two-launch reference and the one-launch result of a shape, computed once."""
    key = (M, K, pad, integer)
    if key not in _CASES:
        o = operands(M, K, pad, integer)
        ref, bufs = two_launches(hip, o, M, K)
        got = one_launch(hip, o, M, K, bufs)
        torch.cuda.synchronize()
        _CASES[key] = (o, ref, bufs, got)
    return _CASES[key]


def test_one_tile_one_stage(hip):
    """The bring-up case: M = 96, K = 32 -- one tile, the prologue's stage alone."""
    _, ref, _, got = case(hip, 96, 32)
    for k in FORMS:
        assert torch.equal(bits(got[k]), bits(ref[k])), k


@pytest.mark.parametrize("pad", (0, 16))
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_one_launch_is_the_two_launches_bit_for_bit(hip, M, K, pad):
    o, ref, _, got = case(hip, M, K, pad)
    assert o["pos"].shape[0] < M or M == 1
    assert torch.isfinite(ref["out"]).all()
    for k in FORMS:                      # whole S3 buffers: the padding rows are compared too
        assert torch.equal(bits(got[k]), bits(ref[k])), (k, M, K, pad)
    # (the forms agree with each other: the S3 outputs hold out and out + pos[row % len])
    assert torch.equal(joined(hip, got["out_s3"], M, 256), got["out"])
    want_p = got["out"] + o["pos"][torch.arange(M, device=DEV) % o["pos"].shape[0]]
    assert torch.equal(joined(hip, got["out_s3_pos"], M, 256), want_p)


@pytest.mark.parametrize("M,K", [(1, 32), (33, 96), (100, 256), (131, 64)])
def test_rows_past_m_are_not_used(hip, M, K):
    """A's allocation holds NaN in every row from M to the next multiple of 96 (and in the pitch
    padding): the outputs, padding rows of CS / CS_pos included, are finite and equal the
    reference, whose split wrote zeros there."""
    o, ref, _, got = case(hip, M, K, 16)
    base = o["a"]._base if o["a"]._base is not None else o["a"]
    assert base.shape[0] % 96 == 0 and torch.isnan(base[M:]).all() and torch.isnan(base[:, K:]).all()
    for k in FORMS:
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(bits(got[k]), bits(ref[k])), k


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_integer_problems_are_exact(hip, M, K):
    """Small-integer operands, gamma = 1, beta = 0: the sums in front of the LayerNorm are integers
    far below 2^24, so the two-launch form holds them exactly (checked: a plain hip.gemm_s3 on the
    split operand equals the fp64 integer result), and the one launch equals the two-launch form
    bit for bit -- the LayerNorm of equal sums.  Against torch's fp64 LayerNorm of the integer
    sums: 2e-5 of the output scale, the bar of the row epilogue's own test
    (tests/test_gemm_s3_gpu.py)."""
    o, ref, bufs, got = case(hip, M, K, integer=True)
    z = o["x"].double() @ o["w"].double().T + o["bias"].double()
    assert (z.abs().max() + 4) < 2 ** 23
    plain = torch.full((M, 256), float("nan"), device=DEV)
    hip.gemm_s3(bufs[0], bufs[1], M, 256, K, bias=o["bias"], out=plain)
    assert torch.equal(plain.double(), z)
    for k in FORMS:
        assert torch.equal(bits(got[k]), bits(ref[k])), (k, M, K)
    want = F_.layer_norm(z + o["res"].double(), (256,), None, None, 1e-5)
    assert (got["out"].double() - want).abs().max() <= 2e-5 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("M,K", [(131, 256), (288, 96)])
def test_two_launches_of_the_kernel_give_equal_bits(hip, M, K):
    o, _, bufs, got = case(hip, M, K)
    again = one_launch(hip, o, M, K, bufs)
    for k in FORMS:
        assert torch.equal(bits(again[k]), bits(got[k])), k


def test_unhandled_shapes_are_refused_without_launching(hip):
    M, K = 96, 64
    o, _, (_, ws, rs), _ = case(hip, M, K)
    out = torch.full((M, 256), 3.0, device=DEV)
    kw = dict(bias=o["bias"], res_s3=rs, gamma=o["gamma"], beta=o["beta"], out=out)
    a = o["a"]
    with pytest.raises(RuntimeError):
        hip.gemm_s3_rows_ln(a, ws, M, 128, K, **kw)                    # N = 128
    with pytest.raises(RuntimeError):
        hip.gemm_s3_rows_ln(a, ws, M, 256, 48, **kw)                   # K = 48
    with pytest.raises(RuntimeError):                                  # lda < K
        hip.gemm_s3_rows_ln(torch.zeros(M, 32, device=DEV), ws, M, 256, K, **kw)
    with pytest.raises(RuntimeError):                                  # lda % 4 != 0
        hip.gemm_s3_rows_ln(torch.zeros(M, K + 2, device=DEV)[:, :K], ws, M, 256, K, **kw)
    with pytest.raises(RuntimeError):                                  # no LayerNorm
        hip.gemm_s3_rows_ln(a, ws, M, 256, K, bias=o["bias"], res_s3=rs, out=out)
    d = hip.GemmS3RowsDesc()                                           # all NULL
    assert hip.lib().pn_gemm_s3_rows_ln_f32(ctypes.byref(d), None) == -1
    torch.cuda.synchronize()
    assert torch.all(out == 3.0)                                       # nothing ran


@pytest.mark.parametrize("K", (16, 256))
@pytest.mark.parametrize("rows", (1, 33, 100))
def test_dual_split_is_the_two_splits_bit_for_bit(hip, rows, K):
    g = torch.Generator().manual_seed(31 * rows + K)
    x = torch.randn(rows, K, generator=g).to(DEV)
    add = torch.randn(max(1, rows // 3), K, generator=g).to(DEV)
    n = hip.s3_floats(rows, K)
    ref_s, ref_p = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    hip.s3_split(x, ref_s)
    hip.s3_split(x, ref_p, add=add)
    got_s, got_p = torch.full((n,), 5.0, device=DEV), torch.full((n,), 5.0, device=DEV)
    hip.s3_split(x, got_s, add=add, out_add=got_p)
    torch.cuda.synchronize()
    assert torch.equal(bits(got_s), bits(ref_s))
    assert torch.equal(bits(got_p), bits(ref_p))
    assert torch.equal(joined(hip, got_s, rows, K), x)


def test_head_encoder_memory_is_the_same_bits_with_and_without_the_row_reading_proj():
    """The 96 x 128 head fixture: pl.X (the encoder's memory) and the head's outputs with
    enc_proj_reads_rows 0 and 1; the switch is part of the stage graphs' configuration."""
    from helpers import head_cfg, oracle_head
    from pairnet_amd import CrossHead2
    _, sd, _ = oracle_head(1234)
    head = CrossHead2(**head_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    assert head.gemm_arithmetic == "bf16x3" and not head.msda_s3_out
    H, W = 96, 128
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(1, c, H // s, W // s, generator=g).to(DEV)
             for c, s in zip((256, 512, 1024, 2048), (4, 8, 16, 32))]
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4)]
    seen = {}
    for rows in (0, 1):
        head.enc_proj_reads_rows = rows
        cls, mask = head.forward(feats, metas)
        torch.cuda.synchronize()
        pl = head._last_plan
        seen[rows] = (pl.X.clone(), pl.graph_cfg, cls["rel"].clone(), mask["mask"].clone())
    assert seen[0][1] != seen[1][1]
    assert torch.isfinite(seen[1][0]).all()
    for i in (0, 2, 3):
        assert torch.equal(bits(seen[0][i]), bits(seen[1][i])), i
