"""GPU: the kernels that do nearly all the arithmetic of a step -- pn_gemm_f32 (its 128x128, 128x64
and 64x64 tile forms, the skinny kernel, the column-major mode, split-K, the grouped launch), the
implicit-GEMM convolution pn_conv2d_nhwc_ex_f32, pn_stem7x7s2_f32, pn_maxpool3x3s2_nhwc_f32, the
Matrix Learner's edge layers and the Winograd transforms -- one at a time against the float64
statements of tests/mm_ref.py (pinned to torch / the oracle without a GPU by tests/test_mm_refs.py)
on the inputs of tests/mm_cases.py.

1. Exact cases.  The fp32 MFMA is exact fp32: on small-integer operands every product and every
   partial sum is exact in any order (test_mm_refs.py proves < 2^24 through every intermediate on
   these very inputs), so the result must equal the statement to the last bit.  This is the
   instrument for index, halo, clamp, tile-overhang and split-start logic.
2. Bounded cases.  |got - ref| <= (L + a) 2^-24 mag + FLT_MIN on every element -- the contract of
   tests/test_fwd_kernels_gpu.py: ref float64, mag the same computation on absolute values, L the
   chain of fp32 roundings counted from the kernel's source (labnotes/r21.md has the formulas,
   written before the first run; mm_cases.chain_* compute them), a = max(4, 2 x the ratio torch's
   own fp32 evaluation reaches on the same inputs).  Nothing in the bound comes from the kernel
   under test.  ReLU and ReLU-after-residual are 1-Lipschitz: no element is left out.
3. Refusals.  PN_BAD_ARG surfaces as RuntimeError before anything is launched; the NaN-filled
   output stays NaN.

Every output is NaN-filled with a NaN fence behind (and, where the call has a leading dimension,
beside) what it may write; every call runs twice and must give equal bits."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import mm_cases as K
import mm_ref as R
import test_fwd_kernels_gpu as FW
from test_fwd_kernels_gpu import _bounded, _is_fence, _nan, _same_bits
from test_grad_kernels_gpu import FLT_MIN, U, _within  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FENCE = 512
NOTED = set()


@pytest.fixture(scope="module")
def hip(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip as h
    h.lib()
    yield h
    print("\n%-26s %12s %14s %10s  case" % ("kernel", "worst ratio", "fp32 oracle", "c"))
    for k in sorted(NOTED & set(FW.WORST)):
        r, o, c, case = FW.WORST[k]
        print("%-26s %12.3f %14.3f %10.4g  %s" % (k, r, o, c, case))


def _d(t):
    return None if t is None else t.to(DEV)


def _fenced(*shape):
    """A NaN-filled buffer of `shape` with FENCE more NaNs behind it -> (view, fence)."""
    n = 1
    for s in shape:
        n *= s
    buf = _nan(n + FENCE)
    return buf[:n].view(*shape), buf[n:]


def _bound(kernel, *a, **kw):
    NOTED.add(kernel)
    return _bounded(kernel, *a, **kw)


def _equal(got, ref64, what):
    """got (fp32, device) equals the float64 statement: no element may differ (the statement's
    values are integers below 2^24, so its fp32 image is itself)."""
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64), what
    g = got.detach().cpu()
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    bad = (g != ref) | torch.isnan(g)
    assert not bool(bad.any()), "%s: %d of %d elements differ, first at %s: got %s, want %s" % (
        what, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()),
        g[bad][:4].tolist(), ref[bad][:4].tolist())


# ============================================================ convolution
def _conv(hip, x, w, bias, res, stride, pad, epi, tile=None, scratch_floats=None, ksplit=0,
          want_splits=None):
    """pn_conv2d_nhwc_ex_f32 twice into fenced NaN outputs -> out [B][Ho][Wo][Cout].  With a
    scratch: NaN-filled, and exactly the first want_splits x B x M x N floats of it are written
    (want_splits = 1: none)."""
    B, H, W_, Cin = x.shape
    Cout, _, KH, KW = w.shape
    Ho, Wo = K.conv_out(H, W_, KH, KW, stride, pad)
    xd, wd, bd, rd = _d(x.contiguous()), _d(K.pack_conv_weight(w)), _d(bias), _d(res)
    outs = []
    for _ in range(2):
        out, fence = _fenced(B, Ho, Wo, Cout)
        scratch = sview = None
        if scratch_floats is not None:
            scratch = _nan(scratch_floats + FENCE)
            sview = scratch[:scratch_floats]
        hip.conv2d_ex(xd, wd, bd, rd, out, B, H, W_, Cin, Cout, KH, KW, stride, pad, tile=tile,
                      scratch=sview, ksplit=ksplit, **K.epilogue_kw(epi))
        torch.cuda.synchronize()
        assert _is_fence(fence), "wrote past the output"
        if scratch is not None:
            used = 0 if want_splits == 1 else want_splits * B * Ho * Wo * Cout
            assert not bool(torch.isnan(scratch[:used]).any()), "fewer splits than the rule gives"
            assert _is_fence(scratch[used:]), "more splits than the rule gives, or past the scratch"
        outs.append(out)
    assert _same_bits(outs[0], outs[1]), "pn_conv2d_nhwc_ex_f32 is not bitwise reproducible"
    return outs[0]


@pytest.mark.parametrize("tile", K.CONV_TILES)
@pytest.mark.parametrize("gi", range(len(K.CONV_GEOMS)))
def test_mm_conv_exact(hip, gi, tile):
    name, H, W, KH, KW, s, p, Cin, Cout = K.CONV_GEOMS[gi]
    epi = K.EPILOGUES[(gi + K.CONV_TILES.index(tile)) % 3]
    x, w, b, res = K.conv_exact(H, W, KH, KW, s, p, Cin, Cout, epi, gi)
    ref, _ = R.conv2d(x, w, b, res, s, p, **K.epilogue_kw(epi))
    _equal(_conv(hip, x, w, b, res, s, p, epi, tile), ref, "%s, tile %s, %s" % (name, tile, epi))


@pytest.mark.parametrize("ci", range(len(K.CONV_SPLITS)))
def test_mm_conv_splitk_exact(hip, ci):
    """Split-K through the convolution loader, the scratch supplied: K.CONV_SPLITS states beside
    each case the chunk every split starts at (on a tap or in the middle of one).  The number of
    splits is the one splitk_factor()'s source gives (restated in mm_cases.splitk, checked on the
    host), seen here as the part of the NaN-filled scratch that was written."""
    name, H, W, k, p, Cin, Cout, forced, S, cps = K.CONV_SPLITS[ci]
    x, w, b, res = K.conv_exact(H, W, k, k, 1, p, Cin, Cout, "after", 40 + ci)
    ref, _ = R.conv2d(x, w, b, res, 1, p, relu_after=True)
    per = K.CONV_B * H * W * Cout
    got = _conv(hip, x, w, b, res, 1, p, "after", None, 16 * per, forced, want_splits=S)
    _equal(got, ref, name)


def test_mm_conv_scratch_too_small_for_two_splits_is_the_single_pass(hip):
    """splitk_factor: S x (B M N) > scratch_floats -> S = scratch_floats / (B M N) = 1 -> one
    pass.  On random operands the split result differs from the single pass in the last bits, so
    equal bits prove which path ran; the scratch stays untouched."""
    name, H, W, k, p, Cin, Cout, forced, S, cps = K.CONV_SPLITS[2]
    x, w, b, res, _ = K.conv_random(H, W, k, k, 1, p, Cin, Cout, "after", "zero", 77)
    per = K.CONV_B * H * W * Cout
    single = _conv(hip, x, w, b, res, 1, p, "after")
    small = _conv(hip, x, w, b, res, 1, p, "after", None, 2 * per - 4, 0, want_splits=1)
    assert _same_bits(single, small)
    split = _conv(hip, x, w, b, res, 1, p, "after", None, 2 * per, 0, want_splits=2)
    assert not _same_bits(single, split), "the split path did not run"


def _conv_o32(x, w, b, res, s, p, epi):
    y = F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=s, padding=p).permute(0, 2, 3, 1)
    y = F.relu(y) if epi == "relu" else y
    y = y + res if res is not None else y
    return F.relu(y) if epi == "after" else y


def _conv_L(K_, epi, splits=1, cps=None):
    """Tile kernels: the fmaf chain over k (K.chain_tile), + bias, + residual."""
    return K.chain_tile(K_, splits, cps) + 1 + (0 if epi == "relu" else 1)


TILE_NAME = {None: "conv 64x64", "128x64": "conv 128x64", "128": "conv 128x128"}


@pytest.mark.parametrize("ci", range(len(K.CONV_BOUNDED)))
def test_mm_conv_bounded(hip, ci):
    gi, tile, epi, kind = K.CONV_BOUNDED[ci]
    name, H, W, KH, KW, s, p, Cin, Cout = K.CONV_GEOMS[gi]
    x, w, b, res, _ = K.conv_random(H, W, KH, KW, s, p, Cin, Cout, epi, kind, 100 + ci)
    ref, mag = R.conv2d(x, w, b, res, s, p, **K.epilogue_kw(epi))
    got = _conv(hip, x, w, b, res, s, p, epi, tile)
    _bound(TILE_NAME[tile], "%s %s %s" % (name, epi, kind), got, ref, mag,
           _conv_L(KH * KW * Cin, epi), _conv_o32(x, w, b, res, s, p, epi))


@pytest.mark.parametrize("ei,mode", [(0, "single"), (1, "single"), (1, "rule"), (1, "ksplit4")])
def test_mm_conv_bounded_short_and_long_chain(hip, ei, mode):
    """The 1x1 convolution at Cin = 32 (L = 32 + bias + residual = 34) and the 7x7 one at
    Cin = 64 (K = 3136, 98 chunks) in one pass, under the rule's six splits of 17 chunks
    (L = 544 + 5 + 2) and under KSPLIT(4): 25 chunks per split (L = 800 + 3 + 2)."""
    name, H, W, KH, KW, s, p, Cin, Cout = K.CONV_BOUNDED_EXTRA[ei]
    x, w, b, res, _ = K.conv_random(H, W, KH, KW, s, p, Cin, Cout, "after", "zero", 150 + ei)
    ref, mag = R.conv2d(x, w, b, res, s, p, relu_after=True)
    per, Kt = K.CONV_B * H * W * Cout, KH * KW * Cin
    if mode == "single":
        S, cps = 1, None
        got = _conv(hip, x, w, b, res, s, p, "after")
    else:
        forced = 4 if mode == "ksplit4" else 0
        S, cps = K.splitk(H * W, Cout, Kt, K.CONV_B, 16 * per, forced)
        assert (S, cps) == ((4, 25) if forced else (6, 17))
        got = _conv(hip, x, w, b, res, s, p, "after", None, 16 * per, forced, want_splits=S)
    _bound("conv 64x64" if S == 1 else "conv split-K", "%s %s" % (name, mode), got, ref, mag,
           _conv_L(Kt, "after", S, cps), _conv_o32(x, w, b, res, s, p, "after"))


# ============================================================ dense contraction
VARIANT = {"skinny": 0, "tile128x64": 2, "tile": 4, "tile64": 6}


def _gemm(hip, A, W, bias, res, force, colmajor=False, aadd=None, from_col=0, relu=False,
          relu_after=False, scratch_floats=None, want_splits=None, variant=None):
    """pn_gemm_f32 on A [Z][M][K], W [Z][N][K] twice -> C [Z][M][N].  Every operand lives in a
    buffer whose rows are 4 (column-major A with M % 4: 3) floats wider than the data, NaN in the
    gap; C is NaN-filled, has such a gap and one spare row per batch entry."""
    Z, M, Kk = A.shape
    N = W.shape[1]
    ldw, ldc, ldres = Kk + 4, N + 4, N + 8
    Wb = _nan(Z, N, ldw)
    Wb[:, :, :Kk] = _d(W)
    if colmajor:
        lda = M + (4 if M % 4 == 0 else 3)
        Ab = _nan(Z, Kk, lda)
        Ab[:, :, :M] = _d(A.transpose(1, 2))
        sA = Kk * lda
    else:
        lda = Kk + 4
        Ab = _nan(Z, M, lda)
        Ab[:, :, :Kk] = _d(A)
        sA = M * lda
    Rb = None
    if res is not None:
        Rb = _nan(Z, M, ldres)
        Rb[:, :, :N] = _d(res)
    kw = dict(M=M, N=N, K=Kk, lda=lda, ldw=ldw, ldc=ldc, bias=_d(bias), res=Rb, ldres=ldres,
              sRes=M * ldres, batch=Z, sA=sA, sW=N * ldw, sC=(M + 1) * ldc, relu=relu,
              relu_after=relu_after, colmajor=colmajor, force=force)
    if aadd is not None:
        Pb = _nan(aadd.shape[0], Kk + 4)
        Pb[:, :Kk] = _d(aadd)
        kw.update(aadd=Pb, ldaadd=Kk + 4, aadd_rows=aadd.shape[0], aadd_from_col=from_col)
    outs = []
    for _ in range(2):
        Cb, fence = _fenced(Z, M + 1, ldc)
        scratch = None
        if scratch_floats is not None:
            scratch = _nan(scratch_floats + FENCE)
            kw["scratch"] = scratch[:scratch_floats]
        if variant is not None:
            got = hip.lib().pn_gemm_variant(C.byref(hip.gemm_desc(Ab, Wb, Cb, **kw)))
            assert got == variant + int(colmajor), (got, variant)
        hip.gemm(Ab, Wb, Cb, **kw)
        torch.cuda.synchronize()
        assert _is_fence(fence) and _is_fence(Cb[:, M]) and _is_fence(Cb[:, :, N:]), \
            "wrote a row past M or a column past N"
        if scratch is not None:
            used = 0 if want_splits == 1 else want_splits * Z * M * N
            assert not bool(torch.isnan(scratch[:used]).any()) and _is_fence(scratch[used:])
        outs.append(Cb[:, :M, :N])
    assert _same_bits(outs[0], outs[1]), "pn_gemm_f32 is not bitwise reproducible"
    return outs[0]


@pytest.mark.parametrize("Kk", K.GEMM_K)
@pytest.mark.parametrize("force", K.GEMM_FORMS + ["tile64"])
def test_mm_gemm_exact(hip, force, Kk):
    """Every M of K.GEMM_M at N = 200 = 3 x 64 + 8 (128-wide tiles: 128 + 72): row-major and
    column-major A (M % 4 != 0: the scalar loader; M % 4 == 0: the vector loader), batches with
    their own W, bias, ReLU, residual, wide lda / ldw / ldc / ldres.  K < 32 must take the skinny
    kernel whatever form is forced.  (tile64 repeats test_gemm_ragged_edges_are_exact's form for
    the column-major loaders, the ragged K and the wide leading dimensions it does not reach.)"""
    variant = VARIANT["skinny" if Kk < 32 else force]
    for M in K.GEMM_M:
        A, W, b, res = K.gemm_exact(M, Kk, M * 1000 + Kk)
        ref, _ = R.gemm(A, W, b, res, relu=True)
        for colmajor in (False, True):
            got = _gemm(hip, A, W, b, res, force, colmajor, relu=True, variant=variant)
            _equal(got, ref, "%s K %d M %d colmajor %d" % (force, Kk, M, colmajor))


@pytest.mark.parametrize("Kk", K.GEMM_K)
@pytest.mark.parametrize("force", K.GEMM_FORMS + ["tile64"])
def test_mm_gemm_aadd_exact(hip, force, Kk):
    """The row-periodic addend: 50 rows under M = 130 (the period does not divide M, and rows 50,
    100 wrap inside a tile), feeding every column and the columns from 64 on only."""
    A, W, b, aadd = K.gemm_aadd_exact(Kk, Kk)
    for from_col in (0, 64):
        ref, _ = R.gemm(A, W, b, None, aadd, from_col)
        got = _gemm(hip, A, W, b, None, force, aadd=aadd, from_col=from_col)
        _equal(got, ref, "%s K %d aadd from column %d" % (force, Kk, from_col))


@pytest.mark.parametrize("Kk", [36, 96, 260])
def test_mm_gemm_group_exact(hip, Kk):
    """Three problems of different M in one grouped launch: bit for bit the single launches and
    the exact product.  (The grouped kernel is the 64x64 tile body: K >= 32.)"""
    probs, refs, fences = [], [], []
    for i, M in enumerate((5, 64, 129)):
        A, W, b, res = K.gemm_exact(M, Kk, 5000 + M + Kk, batch=1 + i % 2)
        Z = A.shape[0]
        aadd = K.ints(K.gen(M), -8, 8, 50, Kk) if i == 2 else None
        refs.append(R.gemm(A, W, b, res, aadd, relu=True)[0])
        Cb, fence = _fenced(Z, M + 1, 204)
        fences.append((Cb, fence, M))
        pr = dict(A=_d(A), W=_d(W), C=Cb, M=M, N=200, K=Kk, lda=Kk, ldw=Kk, ldc=204, batch=Z,
                  sA=M * Kk, sW=200 * Kk, sC=(M + 1) * 204, bias=_d(b), res=_d(res), ldres=200,
                  sRes=M * 200, relu=True)
        if aadd is not None:
            pr.update(aadd=_d(aadd), ldaadd=Kk, aadd_rows=50)
        probs.append(pr)
    hip.gemm_group(probs)
    torch.cuda.synchronize()
    first = [pr["C"].clone() for pr in probs]
    hip.gemm_group(probs)
    torch.cuda.synchronize()
    for pr, ref, (Cb, fence, M), c0 in zip(probs, refs, fences, first):
        assert _same_bits(Cb, c0), "pn_gemm_group_f32 is not bitwise reproducible"
        assert _is_fence(fence) and _is_fence(Cb[:, M]) and _is_fence(Cb[:, :, 200:])
        _equal(Cb[:, :M, :200], ref, "group M %d K %d" % (M, Kk))
        single, _f = _fenced(*Cb.shape)
        kw = {k: v for k, v in pr.items() if k not in ("A", "W", "C")}
        hip.gemm(pr["A"], pr["W"], single, force="tile64", **kw)
        torch.cuda.synchronize()
        assert _same_bits(single, Cb)


def _gemm_o32(A, W, b, res, aadd):
    x = A if aadd is None else A + aadd[torch.arange(A.shape[1]) % aadd.shape[0]]
    return F.relu(torch.einsum("zmk,znk->zmn", x, W) + b) + res


@pytest.mark.parametrize("M,N,Kk,force,colmajor,rows,split", K.GEMM_BOUNDED)
def test_mm_gemm_bounded(hip, M, N, Kk, force, colmajor, rows, split):
    """L: the contraction's chain (K.chain_tile / K.chain_skinny, split-K: the longest slice and
    the S - 1 adds), + 1 where an addend is rounded onto A, + bias, + residual."""
    ci = K.GEMM_BOUNDED.index((M, N, Kk, force, colmajor, rows, split))
    A, W, b, res, aadd, _ = K.gemm_random(M, N, Kk, 200 + ci, aadd_rows=rows)
    ref, mag = R.gemm(A, W, b, res, aadd, relu=True)
    S, cps, floats = 1, None, None
    if split:
        floats = 16 * M * N
        S, cps = K.splitk(M, N, Kk, 1, floats)
        assert (S, cps) == (6, 11)
    got = _gemm(hip, A, W, b, res, force, colmajor, aadd, relu=True, scratch_floats=floats,
                want_splits=S if split else None, variant=VARIANT[force])
    chain = K.chain_skinny(Kk) if force == "skinny" else K.chain_tile(Kk, S, cps)
    name = "gemm split-K" if split else "gemm %s%s" % (force, " A_COL" if colmajor else "")
    _bound(name, "M %d N %d K %d aadd %d" % (M, N, Kk, rows), got, ref, mag,
           chain + (1 if rows else 0) + 2, _gemm_o32(A, W, b, res, aadd))


# ============================================================ stem, max pool, edge layers
def _stem(hip, img, w, b):
    B, _, H, W = img.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    imgd, wd, bd = _d(img.contiguous()), _d(K.pack_stem_weight(w)), _d(b)
    outs = []
    for _ in range(2):
        out, fence = _fenced(B, Ho, Wo, 64)
        hip.stem7x7s2(imgd, wd, bd, out, B, H, W)
        torch.cuda.synchronize()
        assert _is_fence(fence)
        outs.append(out)
    assert _same_bits(outs[0], outs[1])
    return outs[0]


@pytest.mark.parametrize("H,W", K.STEM_HW)
def test_mm_stem_exact(hip, H, W):
    img, w, b = K.stem_exact(H, W, H * 1000 + W)
    _equal(_stem(hip, img, w, b), R.stem(img, w, b)[0], "stem %dx%d" % (H, W))


@pytest.mark.parametrize("H,W,kind", [(7, 9, "zero"), (7, 9, "border"), (9, 65, "zero"),
                                      (10, 130, "border")])
def test_mm_stem_bounded(hip, H, W, kind):
    """L = 151: 75 MFMAs of two taps each, one chain, + bias."""
    img, w, b, _ = K.stem_random(H, W, kind, H)
    ref, mag = R.stem(img, w, b)
    o32 = F.relu(F.conv2d(img, w, b, stride=2, padding=3)).permute(0, 2, 3, 1)
    _bound("k_stem7x7s2", "%dx%d %s" % (H, W, kind), _stem(hip, img, w, b), ref, mag, 151, o32)


@pytest.mark.parametrize("Cc", K.POOL_C)
@pytest.mark.parametrize("kind", K.POOL_KINDS)
def test_mm_maxpool_bitwise(hip, kind, Cc):
    """Every H, W in 1 .. 5: all-negative inputs (a padding of 0 instead of -inf would win at
    every border), a -inf among them, ordinary values."""
    for H in K.POOL_SIDES:
        for W in K.POOL_SIDES:
            x = K.pool_input(H, W, Cc, kind, 10 * H + W)
            ref = R.maxpool3x3s2(x)
            outs = []
            for _ in range(2):
                out, fence = _fenced(*ref.shape)
                hip.maxpool3x3s2(_d(x), out, 2, H, W, Cc)
                torch.cuda.synchronize()
                assert _is_fence(fence)
                outs.append(out)
            assert _same_bits(outs[0], outs[1])
            assert _same_bits(outs[0], _d(ref)), "max pool %dx%d C %d %s" % (H, W, Cc, kind)


def _edges(hip, x1, w1, b1, x3, w3, b3):
    S = x1.shape[1]
    firsts, lasts = [], []
    for _ in range(2):
        o1, f1 = _fenced(2, S * S, 64)
        o3, f3 = _fenced(2, S, S)
        hip.mlearner_first(_d(x1), _d(w1), _d(b1), o1, 2, S)
        hip.mlearner_last(_d(x3), _d(w3), _d(b3), o3, 2, S)
        torch.cuda.synchronize()
        assert _is_fence(f1) and _is_fence(f3)
        firsts.append(o1)
        lasts.append(o3)
    assert _same_bits(firsts[0], firsts[1]) and _same_bits(lasts[0], lasts[1])
    return firsts[0], lasts[0]


@pytest.mark.parametrize("S", K.EDGE_S)
def test_mm_edge_layers_exact(hip, S):
    t = K.edge_exact(S, S)
    first, last = _edges(hip, *t)
    _equal(first, R.mlearner_first(*t[:3])[0], "mlearner_first S %d" % S)
    _equal(last, R.mlearner_last(*t[3:])[0], "mlearner_last S %d" % S)


@pytest.mark.parametrize("S", [5, 17])
def test_mm_edge_layers_bounded(hip, S):
    """k_ml_first: 49 multiply-adds, + bias: L = 50.  k_ml_last: 49 per lane, six butterfly
    steps over the 64 lanes, + bias: L = 56."""
    t = K.edge_random(S, S)
    first, last = _edges(hip, *t)
    x1, w1, b1, x3, w3, b3 = t
    ref, mag = R.mlearner_first(x1, w1, b1)
    o32 = F.relu(F.conv2d(x1[:, None], w1.reshape(64, 1, 7, 7), b1, padding=3))
    _bound("k_ml_first", "S %d" % S, first, ref, mag, 50, o32.permute(0, 2, 3, 1).reshape(2, S * S, 64))
    ref, mag = R.mlearner_last(x3, w3, b3)
    o32 = F.conv2d(x3.permute(0, 3, 1, 2), w3.t().reshape(1, 64, 7, 7), b3, padding=3)[:, 0]
    _bound("k_ml_last", "S %d" % S, last, ref, mag, 56, o32)


# ============================================================ Winograd
WINO_IN = {2: "pn_winograd_f23_input_f32", 4: "pn_winograd_f43_input_f32"}
WINO_OUT = {2: "pn_winograd_f23_output_f32", 4: "pn_winograd_f43_output_f32"}
SPARE_ROWS = 4      # NaN rows behind the last image: a clipped tile row written lands in them


def _wino_input(hip, x, m):
    B, H, W, Cc = x.shape
    th, tw = R.wino_tiles(B, H, W, m)
    xd = _d(x.contiguous())
    outs = []
    for _ in range(2):
        V, fence = _fenced((m + 2) ** 2, B * th * tw, Cc)
        hip._check(getattr(hip.lib(), WINO_IN[m])(hip._ptr(xd), hip._ptr(V), B, H, W, Cc,
                                                  hip._stream()), WINO_IN[m])
        torch.cuda.synchronize()
        assert _is_fence(fence)
        outs.append(V)
    assert _same_bits(outs[0], outs[1])
    return outs[0]


def _wino_output(hip, Mx, bias, B, H, W, m, relu):
    """-> out [B][H][W][C]; behind it SPARE_ROWS image rows of NaN and the usual fence."""
    Cc = Mx.shape[2]
    bd = _d(bias)
    outs = []
    for _ in range(2):
        buf, fence = _fenced(B * H + SPARE_ROWS, W, Cc)
        hip._check(getattr(hip.lib(), WINO_OUT[m])(hip._ptr(Mx), hip._ptr(bd), hip._ptr(buf), B, H,
                                                   W, Cc, int(relu), hip._stream()), WINO_OUT[m])
        torch.cuda.synchronize()
        assert _is_fence(fence) and _is_fence(buf[B * H:]), "a clipped tile row was written"
        outs.append(buf[:B * H].view(B, H, W, Cc))
    assert _same_bits(outs[0], outs[1])
    return outs[0]


def _wino_conv(hip, x, w, bias, m, relu):
    """The three launches of hip.conv3x3_winograd / _winograd43 with the device weight transform,
    every buffer NaN-filled and fenced."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    th, tw = R.wino_tiles(B, H, W, m)
    T, P = B * th * tw, (m + 2) ** 2
    Ud = (hip.winograd_weights if m == 2 else hip.winograd43_weights)(_d(w))
    run = hip.conv3x3_winograd if m == 2 else hip.conv3x3_winograd43
    xd, bd = _d(x.contiguous()), _d(bias)
    outs = []
    for _ in range(2):
        V, fv = _fenced(P, T, Cin)
        Mb, fm = _fenced(P, T, Cout)
        buf, fence = _fenced(B * H + SPARE_ROWS, W, Cout)
        run(xd, Ud, bd, buf, V, Mb, B, H, W, Cin, Cout, relu)
        torch.cuda.synchronize()
        assert _is_fence(fv) and _is_fence(fm) and _is_fence(fence) and _is_fence(buf[B * H:])
        outs.append(buf[:B * H].view(B, H, W, Cout))
    assert _same_bits(outs[0], outs[1])
    return outs[0]


WINO_EXACT = [(m, H, W, ci, co) for m in (2, 4) for (H, W) in K.WINO_HW[m] for (ci, co) in K.WINO_CH[m]]


@pytest.mark.parametrize("m,H,W,Cin,Cout", WINO_EXACT)
def test_mm_winograd_exact(hip, m, H, W, Cin, Cout):
    """Integer operands, U integral: the device weight transform against the double statement,
    the input and the output transform alone against B^T d B and A^T M A, and the composition
    against the exact direct convolution -- all to the last bit."""
    x, w, b = K.wino_exact(m, H, W, Cin, Cout, H * 16 + W)
    Ud = (hip.winograd_weights if m == 2 else hip.winograd43_weights)(_d(w))
    _equal(Ud, R.wino_weights(w, m), "weight transform F(%d,3)" % m)
    _equal(_wino_input(hip, x, m), R.wino_input(x, m), "input transform")
    Mx, bias = K.wino_m_exact(m, H, W, Cout, H + W)
    for relu in (False, True):
        _equal(_wino_output(hip, _d(Mx), bias, K.WINO_B, H, W, m, relu),
               R.wino_output(Mx, bias, K.WINO_B, H, W, m, relu), "output transform relu %d" % relu)
    relu = bool((H + W) % 2)
    direct, _ = R.conv2d(x, w, b, None, 1, 1, relu=relu)
    _equal(_wino_conv(hip, x, w, b, m, relu), direct, "F(%d,3) %dx%d %d -> %d" % (m, H, W, Cin, Cout))


@pytest.mark.parametrize("m,H,W,Cin,Cout,relu,kind", K.WINO_BOUNDED)
def test_mm_winograd_bounded(hip, m, H, W, Cin, Cout, relu, kind):
    """ref: the direct float64 convolution; mag: the Winograd statement on absolute values.
    L = in + 1 + chain + out with the GEMM's chain over Cin (the longer of the tile and the skinny
    form), one rounding of U, and the transforms' roundings
      F(2,3): in 2 (one subtraction per side), out 2 + 2 adds and the bias = 5
      F(4,3): in 4 (bt6: two fused steps per side), out 3 per side (at6) and the bias = 7."""
    x, w, b, _ = K.wino_random(m, H, W, Cin, Cout, kind, 300 + H * 16 + W)
    ref, _ = R.conv2d(x, w, b, None, 1, 1, relu=relu)
    _, mag, _ = R.wino_conv(x, w, b, m)
    chain = max(K.chain_tile(Cin), K.chain_skinny(Cin))
    L = (2 + 1 + chain + 5) if m == 2 else (4 + 1 + chain + 7)
    o32 = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1)
    _bound("winograd F(%d,3)" % m, "%dx%d %d -> %d relu %d %s" % (H, W, Cin, Cout, relu, kind),
           _wino_conv(hip, x, w, b, m, relu), ref, mag, L, F.relu(o32) if relu else o32)


# ============================================================ refusals
def _refused(call, *fenced):
    with pytest.raises(RuntimeError, match="argument contract violated"):
        call()
    torch.cuda.synchronize()
    for t in fenced:
        assert _is_fence(t), "a refused call wrote its output"


def _z(*shape):
    return torch.zeros(*shape, device=DEV)


@pytest.mark.parametrize("KH,KW,pad", [(1, 1, 1), (2, 2, 1), (1, 3, 1)])
def test_mm_conv_refuses_a_pad_beyond_the_kernel(hip, KH, KW, pad):
    """2 pad > min(KH, KW) - 1: the loader reads pixel (oy stride, ox stride) in place of a tap
    outside the image, and that pixel would lie outside it too."""
    B, H, W, Cc = 2, 4, 4, 32
    Ho, Wo = K.conv_out(H, W, KH, KW, 1, pad)
    for tile in K.CONV_TILES:
        out = _nan(B * Ho * Wo * Cc + FENCE)
        _refused(lambda: hip.conv2d_ex(_z(B, H, W, Cc), _z(Cc, KH * KW * Cc), _z(Cc), None, out, B,
                                       H, W, Cc, Cc, KH, KW, 1, pad, tile=tile), out)


def test_mm_conv_refusals(hip):
    B, H, W, Cc = 2, 4, 4, 32
    out = _nan(B * H * W * Cc + FENCE)
    x, w, b = _z(B, H, W, Cc + 4), _z(Cc, 9 * Cc + 4), _z(Cc)
    # Cin % 32
    _refused(lambda: hip.conv2d_ex(_z(B, H, W, 16), _z(Cc, 9 * 16), b, None, out, B, H, W, 16, Cc,
                                   3, 3, 1, 1), out)
    # a non-positive Ho: 4 rows under a 7-row kernel without padding
    _refused(lambda: hip.conv2d_ex(x, _z(Cc, 49 * Cc), b, None, out, B, H, W, Cc, Cc, 7, 7, 1, 0), out)
    _refused(lambda: hip.conv2d_ex(x, _z(Cc, 49 * Cc), b, None, out, B, H, W, Cc, Cc, 7, 7, 2, 0), out)
    # misaligned input / weights
    _refused(lambda: hip.conv2d_ex(x.view(-1)[1:], w, b, None, out, B, H, W, Cc, Cc, 3, 3, 1, 1), out)
    _refused(lambda: hip.conv2d_ex(x, w.view(-1)[2:], b, None, out, B, H, W, Cc, Cc, 3, 3, 1, 1), out)
    # the "same" entry refuses what is not 2 pad + 1
    _refused(lambda: hip.conv2d_nhwc(x, w, b, out, B, H, W, Cc, Cc, 3, 3, 0, False), out)


def test_mm_gemm_refusals(hip):
    M, N, Kk = 8, 64, 32
    out = _nan(M * N + FENCE)
    A, W, P = _z(M + 1, Kk + 8), _z(N + 1, Kk + 8), _z(4, Kk)
    ok = dict(M=M, N=N, K=Kk, lda=Kk, ldw=Kk, ldc=N)
    for bad in (dict(K=30), dict(lda=Kk + 2), dict(ldw=Kk + 2),
                dict(aadd=P, ldaadd=Kk, aadd_rows=4, aadd_from_col=32),
                dict(aadd=P, ldaadd=Kk, aadd_rows=4, colmajor=True, lda=M),
                dict(aadd=P, ldaadd=Kk, aadd_rows=0)):
        for force in (None, "tile", "tile64", "tile128x64", "skinny"):
            _refused(lambda: hip.gemm(A, W, out, force=force, **dict(ok, **bad)), out)
    _refused(lambda: hip.gemm(A.view(-1)[1:], W, out, **ok), out)
    _refused(lambda: hip.gemm(A, W.view(-1)[1:], out, **ok), out)
    # a group of GEMM_GROUP_MAX + 1, and a column-major member
    pr = dict(A=A, W=W, C=out, **ok)
    assert hip.GEMM_GROUP_MAX == K.GEMM_GROUP_MAX
    _refused(lambda: hip.gemm_group([pr] * (hip.GEMM_GROUP_MAX + 1)), out)
    _refused(lambda: hip.gemm_group([pr, dict(pr, colmajor=True, lda=M)]), out)
    # K < 32 has no tile form (pn_gemm_f32 sends it to the skinny kernel; a group cannot)
    _refused(lambda: hip.gemm_group([pr, dict(pr, K=28, lda=28, ldw=28)]), out)


def test_mm_transform_pool_and_edge_refusals(hip):
    lib, ptr, st = hip.lib(), hip._ptr, hip._stream
    out, x = _nan(4096 + FENCE), _z(4096)
    for (H, W, Cc) in ((1, 4, 4), (4, 1, 4), (4, 4, 6)):        # F(2,3): H, W >= 2 and C % 4 == 0
        _refused(lambda: hip._check(lib.pn_winograd_f23_input_f32(ptr(x), ptr(out), 1, H, W, Cc,
                                                                  st()), "f23 input"), out)
        _refused(lambda: hip._check(lib.pn_winograd_f23_output_f32(ptr(x), None, ptr(out), 1, H, W,
                                                                   Cc, 0, st()), "f23 output"), out)
    _refused(lambda: hip._check(lib.pn_winograd_f43_input_f32(ptr(x), ptr(out), 1, 4, 4, 6, st()),
                                "f43 input"), out)
    _refused(lambda: hip._check(lib.pn_winograd_f43_output_f32(ptr(x), None, ptr(out[1:]), 1, 4, 4,
                                                               4, 0, st()), "f43 output"), out)
    _refused(lambda: hip._check(lib.pn_winograd_weights_f32(ptr(x), ptr(out), 4, 4, 3, st()),
                                "weights"), out)
    _refused(lambda: hip.maxpool3x3s2(x, out, 2, 4, 4, 6), out)
    _refused(lambda: hip.maxpool3x3s2(x[1:], out, 2, 4, 4, 4), out)
    for Cc in (32, 63, 128):                                     # the edge layers: C == 64 only
        _refused(lambda: hip._check(lib.pn_mlearner_first_f32(ptr(x), ptr(x), ptr(x), ptr(out), 1, 4,
                                                              Cc, st()), "first"), out)
        _refused(lambda: hip._check(lib.pn_mlearner_last_f32(ptr(x), ptr(x), ptr(x), ptr(out), 1, 4,
                                                             Cc, st()), "last"), out)
