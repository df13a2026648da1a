"""GPU: the two entries of csrc/fpn_grad.hip alone, against the float64 statements of
tests/fpn_grad_ref.py, with the bound of labnotes R14.2 / R19.2:

    |got - ref| <= (L + a + cond) 2^-24 mag + 2^-24 extra + FLT_MIN

  L      roundings on the longest path, counted from the kernel's source (below, per kernel)
  mag    the float64 computation on absolute values
  a      max(4, 2 x the ratio torch's fp32 evaluation of the same statement reaches on the inputs)
  cond   GroupNorm: the double statistics' share (fpn_grad_ref.group_norm_bwd, `cnt_stats`)
  extra  adjoint: 3 (1 + in) 2^-24 of a pixel per axis times sum |g| over the candidate window

Nothing in a bound comes from the kernel under test.  Untouched outputs, NaN fences, repeated runs,
the identity and the integer case are compared bitwise.

pn_bilinear_nhwc_bwd_f32, per coarse element with ny x nx candidates: l1 = src - i0 and
l0 = 1 - l1 (2 per axis), l0 + l1 at the clamped index (1), an fmaf per contributing column (nx),
an fmaf per contributing row (ny): L = nx + ny + 5, + 1 when accumulating.
pn_groupnorm_act_nhwc_bwd_f32: dx: xhat (subtraction, product: 2), gamma dy (1), - m1 (1),
xhat m2 and its subtraction (2), rstd (1), and the four statistics rounded to fp32 with rstd used
twice (5): L = 12.  d gamma: dy xhat (2 + 1, mean and rstd rounded: 2), 16 fp32 adds per thread, 16
across the workgroup, the double sum's rounding and the accumulate: L = 39; d beta: L = 34."""
import pytest
import torch
import torch.nn.functional as F

import fpn_grad_ref as R
from test_fwd_kernels_gpu import (DEV, NAN, _bounded, _d, _is_fence, _nan, _same_bits)  # noqa: F401
from test_fwd_kernels_gpu import WORST

pytestmark = pytest.mark.gpu
SIZES = [(1, 1, 1, 1), (1, 1, 3, 5), (5, 5, 5, 5), (8, 12, 16, 24), (7, 10, 13, 19), (3, 4, 5, 7),
         (2, 3, 9, 4)]
GN_L_DX, GN_L_DG, GN_L_DB = 12, 39, 34


@pytest.fixture(scope="module")
def hip(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip as h
    h.lib()
    yield h
    print("\n%-32s %12s %14s %10s  case" % ("kernel", "worst ratio", "fp32 oracle", "c"))
    for k, (r, o, c, case) in sorted(WORST.items()):
        if "bwd" in k:
            print("%-32s %12.3f %14.3f %10.4g  %s" % (k, r, o, c, case))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nhwc(t):                                   # [B, C, h, w] -> [B, h * w, C]
    B, C, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(B, h * w, C)


def _adjoint(hip, g_nhwc, B, hi, wi, ho, wo, C, acc, base=None, pad_o=5, pad_i=3):
    """One fenced launch: both batch strides larger than the maps -> the coarse rows [B, hi*wi, C]."""
    gin = _nan(B, ho * wo + pad_o, C)
    gin[:, :ho * wo] = g_nhwc
    out = _nan(B, hi * wi + pad_i, C)
    if acc:
        out[:, :hi * wi] = base
    hip.bilinear_nhwc_bwd(gin, out, B, hi, wi, ho, wo, C, acc, (ho * wo + pad_o) * C,
                          (hi * wi + pad_i) * C)
    torch.cuda.synchronize()
    assert _is_fence(out[:, hi * wi:])
    return out[:, :hi * wi]


@pytest.mark.parametrize("C", [4, 256])
@pytest.mark.parametrize("hi,wi,ho,wo", SIZES)
def test_bilinear_adjoint_against_the_statement(hip, hi, wi, ho, wo, C):
    B = 2
    gen = _gen(hi * 1000 + wo * 10 + C)
    g = torch.randn(B, C, ho, wo, generator=gen) * 2.0
    base = _d(torch.randn(B, hi * wi, C, generator=gen))
    ref, mag, extra = R.bilinear_adjoint(_d(g), hi, wi)
    x32 = torch.zeros(B, C, hi, wi, device=DEV, requires_grad=True)
    o32, = torch.autograd.grad(F.interpolate(x32, size=(ho, wo), mode="bilinear",
                                             align_corners=False), x32, _d(g))
    L = R.adjoint_contributors(hi, ho) + R.adjoint_contributors(wi, wo) + 5
    case = "%dx%d -> %dx%d C=%d" % (hi, wi, ho, wo, C)
    for acc in (False, True):
        outs = [_adjoint(hip, _d(_nhwc(g)), B, hi, wi, ho, wo, C, acc, base) for _ in range(2)]
        assert _same_bits(outs[0], outs[1])                         # two runs: the same bits
        r, m_, o = _nhwc(ref), _nhwc(mag), _nhwc(o32)
        if acc:
            r, m_, o = r + base.double(), m_ + base.double().abs(), o + base
        _bounded("k_bilinear_nhwc_bwd", case + (" accumulate" if acc else ""), outs[0], r, m_,
                 L + int(acc), o, extra=_nhwc(extra))
        if (hi, wi) == (ho, wo) and not acc:
            assert _same_bits(outs[0], _d(_nhwc(g)))                # identity, bit for bit


def test_bilinear_adjoint_of_small_integers_is_exact(hip):
    """8x12 -> 16x24: every tap weight is a multiple of 1/4 and exact in fp32, so with small
    integer g every product and partial sum is exact: the statement, bit for bit."""
    B, C = 2, 256
    g = torch.randint(-8, 9, (B, C, 16, 24), generator=_gen(3)).float()
    ref, _, _ = R.bilinear_adjoint(_d(g), 8, 12)
    got = _adjoint(hip, _d(_nhwc(g)), B, 8, 12, 16, 24, C, False)
    assert _same_bits(got, _nhwc(ref).float())


@pytest.mark.parametrize("hi,wi,ho,wo", [(8, 12, 16, 24), (7, 10, 13, 19), (2, 3, 9, 4)])
def test_bilinear_adjoint_is_the_transpose_of_the_forward_kernel(hip, hi, wi, ho, wo):
    """<up(x), g> = <x, adj(g)> with `up` the existing pn_bilinear_nhwc_f32: both sides are sums of
    ho wo C (hi wi C) products of fp32 values; the difference is bounded by each side's own bound
    summed over its elements."""
    B, C = 2, 256
    gen = _gen(77 + hi)
    x, g = torch.randn(B, C, hi, wi, generator=gen), torch.randn(B, C, ho, wo, generator=gen)
    up = _nan(B, ho * wo, C)
    hip.bilinear_nhwc(_d(_nhwc(x)).contiguous(), up, B, hi, wi, ho, wo, C, False, hi * wi * C,
                      ho * wo * C)
    adj = _adjoint(hip, _d(_nhwc(g)), B, hi, wi, ho, wo, C, False)
    lhs = float((up.double() * _d(_nhwc(g)).double()).sum())
    rhs = float((_d(_nhwc(x)).double() * adj.double()).sum())
    import fwd_cases as K
    import fwd_ref as FR
    _, fmag, spread = FR.bilinear(_d(x), ho, wo)
    _, amag, aextra = R.bilinear_adjoint(_d(g), hi, wi)
    La = R.adjoint_contributors(hi, ho) + R.adjoint_contributors(wi, wo) + 5
    bound = R.U * (float(((K.BIL_L + 4) * fmag + K.bilinear_extra(hi, wi, spread)).mul(_d(g).double().abs()).sum())
                   + float((((La + 4) * amag + aextra) * _d(x).double().abs()).sum()))
    print("<up x, g> = %.9e, <x, adj g> = %.9e, |difference| %.3e (bound %.3e)"
          % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


def test_bilinear_adjoint_refusals(hip):
    lib = hip.lib()
    g, out = _nan(2, 16 * 24, 8), _nan(2, 8 * 12, 8)
    p, q = g.data_ptr(), out.data_ptr()
    ok = (p, q, 2, 8, 12, 16, 24, 8, 0, 16 * 24 * 8, 8 * 12 * 8, None)
    bad = [(None,) + ok[1:], (p, None) + ok[2:],
           (p, q, 0) + ok[3:], (p, q, 2, 0) + ok[4:], (p, q, 2, 8, 0) + ok[5:],
           (p, q, 2, 8, 12, 0) + ok[6:], (p, q, 2, 8, 12, 16, -1) + ok[7:],
           (p, q, 2, 8, 12, 7, 24) + ok[7:],                 # ho < hi
           (p, q, 2, 8, 12, 16, 11) + ok[7:],                # wo < wi
           (p, q, 2, 8, 12, 16, 24, 6) + ok[8:],             # C & 3
           (p, q, 2, 8, 12, 16, 24, 0) + ok[8:],
           ok[:9] + (16 * 24 * 8 + 2,) + ok[10:],            # batch strides not multiples of 4
           ok[:10] + (8 * 12 * 8 + 1,) + ok[11:]]
    for i, args in enumerate(bad):
        assert lib.pn_bilinear_nhwc_bwd_f32(*args) == -1, i
    torch.cuda.synchronize()
    assert _is_fence(out)


# ============================================================ GroupNorm (+ReLU) backward
def _gn_case(hip, B, HW, G, relu, seed, offset=False, accumulate=False):
    gen = _gen(seed)
    x = torch.randn(B, HW, 256, generator=gen)
    if offset:
        x = 1000.0 + 0.01 * x
    dy = torch.randn(B, HW, 256, generator=gen)
    gamma, beta = torch.randn(256, generator=gen), torch.randn(256, generator=gen)
    x, dy, gamma, beta = _d(x), _d(dy), _d(gamma), _d(beta)
    y = gate = None
    if relu:
        y = F.relu(F.group_norm(x.permute(0, 2, 1), G, gamma, beta, 1e-5)).permute(0, 2, 1).contiguous()
        gate = (y > 0).float()
    ref = R.group_norm_bwd(x, dy, gamma, G, 1e-5, gate)
    o32 = R.group_norm_bwd(x, dy, gamma, G, 1e-5, gate, dtype=torch.float32)
    base_g = _d(torch.randn(256, generator=gen)) if accumulate else None
    base_b = _d(torch.randn(256, generator=gen)) if accumulate else None
    xin, din = _nan(B, HW + 3, 256), _nan(B, HW + 5, 256)          # batch strides on both inputs
    xin[:, :HW], din[:, :HW] = x, dy
    nblk = hip.groupnorm_nblk(HW)
    runs = []
    for _ in range(2):
        dx, stats = _nan(B * HW + 1, 256), _nan(B * G * 4 + 4)
        part = torch.full((B * nblk * G * 4 + 8,), NAN, device=DEV, dtype=torch.float64)
        col = _nan(B * nblk * 512 + 8)
        dgb = _nan(3, 256)                                          # d gamma | d beta | fence
        if accumulate:
            dgb[0], dgb[1] = base_g, base_b
        hip.groupnorm_act_nhwc_bwd(xin, din, y, gamma, dx[:B * HW], dgb[0], dgb[1], stats,
                                   (part, col), B, HW, G, relu, accumulate, (HW + 3) * 256,
                                   (HW + 5) * 256)
        torch.cuda.synchronize()
        assert _is_fence(dx[B * HW:]) and _is_fence(stats[B * G * 4:]) and _is_fence(dgb[2])
        assert bool(torch.isnan(part[B * nblk * G * 4:]).all()) and _is_fence(col[B * nblk * 512:])
        assert bool(torch.isfinite(part[:B * nblk * G * 4]).all())
        runs.append((dx[:B * HW].view(B, HW, 256), dgb[0].clone(), dgb[1].clone(), stats[:B * G * 4]))
    for a, b in zip(*runs):
        assert _same_bits(a, b)                                     # bitwise repeatable
    case = "HW=%d G=%d relu=%d%s%s" % (HW, G, relu, " offset" if offset else "",
                                       " accumulate" if accumulate else "")
    dx, dg, db, _ = runs[0]
    cs = ref["cnt_stats"]
    _bounded("k_gnact_bwd dx", case, dx, ref["dx"], ref["dx_mag"], GN_L_DX, o32["dx"], cond=2 * cs)
    rg, mg, og = ref["dgamma"], ref["dgamma_mag"], o32["dgamma"]
    rb, mb, ob = ref["dbeta"], ref["dbeta_mag"], o32["dbeta"]
    if accumulate:
        rg, mg, og = rg + base_g.double(), mg + base_g.double().abs(), og + base_g
        rb, mb, ob = rb + base_b.double(), mb + base_b.double().abs(), ob + base_b
    _bounded("k_gnact_bwd dgamma", case, dg, rg, mg, GN_L_DG, og, cond=cs)
    _bounded("k_gnact_bwd dbeta", case, db, rb, mb, GN_L_DB, ob)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("G", [32, 4])
@pytest.mark.parametrize("HW", [1, 255, 256, 257, 700])
def test_groupnorm_act_backward_against_the_statement(hip, HW, G, relu):
    """HW: one pixel; one below, at and one above the 256-pixel block boundary of
    pn_groupnorm_nblk; three blocks with a ragged last one.  B = 2, strided inputs."""
    assert hip.groupnorm_nblk(256) == 1 and hip.groupnorm_nblk(257) == 2 and hip.groupnorm_nblk(700) == 3
    _gn_case(hip, 2, HW, G, relu, seed=HW * 10 + G + relu)


def test_groupnorm_act_backward_offset_rows_and_accumulate(hip):
    _gn_case(hip, 2, 257, 32, True, seed=5, offset=True)          # rows 1000 + 0.01 noise
    _gn_case(hip, 2, 300, 32, True, seed=6, accumulate=True)      # into non-zero d gamma / d beta
    _gn_case(hip, 2, 300, 4, False, seed=7, accumulate=True)


def test_groupnorm_act_backward_refusals(hip):
    lib = hip.lib()
    t = _nan(2, 64, 256)
    dx, st, col, dg, db = _nan(2 * 64, 256), _nan(2 * 32 * 4), _nan(2 * 512), _nan(256), _nan(256)
    part = torch.full((2 * 32 * 4,), NAN, device=DEV, dtype=torch.float64)
    p = t.data_ptr()
    ok = [p, p, p, p, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), st.data_ptr(), part.data_ptr(),
          col.data_ptr(), 2, 64, 32, 1e-5, 1, 0, 64 * 256, 64 * 256, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.pn_groupnorm_act_nhwc_bwd_f32(*a)

    for i in (0, 1, 3, 4, 5, 6, 7, 8, 9):                          # a null pointer
        assert call(**{"a%d" % i: None}) == -1, i
    assert call(a2=None) == -1                                     # relu needs the saved output
    for kw in (dict(a10=0), dict(a10=65536), dict(a11=0), dict(a11=2 ** 31), dict(a12=0),
               dict(a12=3), dict(a12=64), dict(a12=128),           # 256 % G, 4-channel lanes
               dict(a16=64 * 256 + 2), dict(a17=64 * 256 + 1)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert _is_fence(dx) and _is_fence(st) and _is_fence(dg) and _is_fence(db) and _is_fence(col)
