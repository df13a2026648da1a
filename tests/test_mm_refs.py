"""Host checks of tests/mm_ref.py and tests/mm_cases.py (no GPU): every float64 statement against
torch in float64 (1e-12: F.conv2d, F.max_pool2d, F.linear / einsum, oracle.matrix_learner for the
edge layers; the Winograd statements against the direct convolution at 1e-10 of mag), and every
condition tests/test_mm_kernels_gpu.py relies on, from the reference alone: the integer cases stay
below 2^24 through every intermediate on the actual seeded inputs, the planted outputs cancel
(|ref| < 1e-6 mag) among ordinary neighbours, the border rows dominate, the split-K rule restated
in mm_cases gives the split counts written beside the cases, and every convolution caller of the
package keeps 2 pad <= K - 1."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import mm_cases as K
import mm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(a, b, tol=1e-12, scale=None):
    scale = float(b.abs().max().clamp_min(1.0)) if scale is None else scale
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert a.shape == b.shape and err <= tol * scale, (a.shape, b.shape, err, scale)


def _torch_conv(x, w, bias, res, stride, pad, relu, relu_after):
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), stride=stride,
                 padding=pad).permute(0, 2, 3, 1)
    y = F.relu(y) if relu else y
    y = y + res.double() if res is not None else y
    return F.relu(y) if relu_after else y


# ------------------------------------------------------------------------------ statements
@pytest.mark.parametrize("gi", range(len(K.CONV_GEOMS)))
def test_conv_statement_is_torch_conv2d(gi):
    name, H, W, KH, KW, s, p, Cin, Cout = K.CONV_GEOMS[gi]
    epi = K.EPILOGUES[gi % 3]
    x, w, b, res, _ = K.conv_random(H, W, KH, KW, s, p, Cin, Cout, epi, "zero", gi)
    ref, mag = R.conv2d(x, w, b, res, s, p, **K.epilogue_kw(epi))
    _close(ref, _torch_conv(x, w, b, res, s, p, **K.epilogue_kw(epi)),
           scale=float(mag.max()))
    want = _torch_conv(x.abs(), w.abs(), b.abs(), None if res is None else res.abs(), s, p,
                       False, False)
    _close(mag, want)
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


def test_gemm_statement_is_torch_linear():
    A, W, b, res, aadd, _ = K.gemm_random(130, 200, 36, 3, batch=2, aadd_rows=50)
    pos = aadd.double().repeat(3, 1)[:130]
    for from_col in (0, 64):
        ref, mag = R.gemm(A, W, b, res, aadd, from_col, relu=True, relu_after=True)
        lo = torch.einsum("zmk,znk->zmn", A.double(), W.double())
        hi = torch.einsum("zmk,znk->zmn", A.double() + pos, W.double())
        y = torch.cat([lo[..., :from_col], hi[..., from_col:]], -1) + b.double()
        _close(ref, F.relu(F.relu(y) + res.double()), scale=float(mag.max()))
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
    ref, mag = R.gemm(A[:1], W[0], b)
    _close(ref[0], F.linear(A[0].double(), W[0].double(), b.double()), scale=float(mag.max()))
    _close(mag[0], F.linear(A[0].double().abs(), W[0].double().abs(), b.double().abs()))


@pytest.mark.parametrize("H,W", [(7, 9), (9, 65)])
def test_stem_statement_is_torch_conv2d(H, W):
    img, w, b, _ = K.stem_random(H, W, "zero", H)
    ref, mag = R.stem(img, w, b)
    want = F.relu(F.conv2d(img.double(), w.double(), b.double(), stride=2, padding=3))
    _close(ref, want.permute(0, 2, 3, 1), scale=float(mag.max()))
    assert K.pack_stem_weight(w)[:, 147:].abs().max() == 0
    assert torch.equal(K.pack_stem_weight(w)[5, 49 + 2 * 7 + 3], w[5, 1, 2, 3])


@pytest.mark.parametrize("kind", K.POOL_KINDS)
def test_maxpool_statement_is_torch_max_pool2d(kind):
    for H in K.POOL_SIDES:
        for W in K.POOL_SIDES:
            x = K.pool_input(H, W, 4, kind, 10 * H + W)
            want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
            assert torch.equal(R.maxpool3x3s2(x), want), (H, W)
            if kind != "ordinary":       # a kernel that padded with 0 would answer 0 somewhere
                assert bool((x < 0).all()) and bool((want < 0).all())
            if kind == "neginf":
                assert bool(torch.isinf(x).any())
    assert bool(torch.isinf(R.maxpool3x3s2(K.pool_input(1, 1, 4, "neginf", 0))[0]).all())


@pytest.mark.parametrize("S", K.EDGE_S)
def test_edge_layer_statements_are_the_oracle(S):
    from oracle.matrix_learner import MatrixLearnerTiny
    x1, w1, b1, x3, w3, b3 = K.edge_random(S, S)
    net = MatrixLearnerTiny().double()
    with torch.no_grad():
        net.conv_layers[0][0].weight.copy_(w1.reshape(64, 1, 7, 7))
        net.conv_layers[0][0].bias.copy_(b1)
        net.conv_layers[2][0].weight.copy_(w3.t().reshape(1, 64, 7, 7))
        net.conv_layers[2][0].bias.copy_(b3)
        c1 = F.relu(net.conv_layers[0][0](x1.double()[:, None]))           # [B][64][S][S]
        y = net.conv_layers[2][0](x3.double().permute(0, 3, 1, 2))[:, 0]
    ref, mag = R.mlearner_first(x1, w1, b1)
    _close(ref, c1.permute(0, 2, 3, 1).reshape(2, S * S, 64), scale=float(mag.max()))
    ref, mag = R.mlearner_last(x3, w3, b3)
    _close(ref, y, scale=float(mag.max()))


@pytest.mark.parametrize("m", [2, 4])
def test_winograd_statements_are_the_direct_convolution(m):
    for (H, W) in K.WINO_HW[m]:
        Cin, Cout = K.WINO_CH[m][0]
        x, w, b, _ = K.wino_random(m, H, W, Cin, Cout, "zero", H * 16 + W)
        direct, _ = R.conv2d(x, w, b, None, 1, 1)
        out, mag, _ = R.wino_conv(x, w, b, m, round_u=False)
        assert float(((out - direct).abs() / mag).max()) <= 1e-10, (m, H, W)
        # with U rounded to fp32 once, at the integer cases' weights (U integral): still exact
        x, w, b = K.wino_exact(m, H, W, Cin, Cout, H * 16 + W)
        direct, _ = R.conv2d(x, w, b, None, 1, 1, relu=True)
        out, mag, _ = R.wino_conv(x, w, b, m, relu=True)
        assert float(((out - direct).abs() / mag.clamp_min(1.0)).max()) <= 1e-10, (m, H, W)
        Ue = torch.einsum("ik,ockl,jl->ijoc", R.G[m], w.double(), R.G[m]).reshape((m + 2) ** 2, Cout, Cin)
        _close(R.wino_weights(w, m, round_u=False), Ue)
        # the parts: input transform of a patch written out, output transform clipped
        V = R.wino_input(x, m)
        d = R.wino_patches(x, m)
        assert torch.equal(V[1 * (m + 2) + 2, 0],
                           (d[0].permute(2, 0, 1) @ R.BT[m][2]) @ R.BT[m][1])
        assert R.wino_output(R.wino_gemm(V, R.wino_weights(w, m)), b, K.WINO_B, H, W, m).shape == \
            (K.WINO_B, H, W, Cout)


# ------------------------------------------------------------------------------ exactness < 2^24
@pytest.mark.parametrize("gi", range(len(K.CONV_GEOMS)))
def test_exact_convolutions_stay_below_2_24(gi):
    name, H, W, KH, KW, s, p, Cin, Cout = K.CONV_GEOMS[gi]
    for epi in K.EPILOGUES:
        x, w, b, res = K.conv_exact(H, W, KH, KW, s, p, Cin, Cout, epi, gi)
        for t in (x, w, b) + (() if res is None else (res,)):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 8
        ref, mag = R.conv2d(x, w, b, res, s, p, **K.epilogue_kw(epi))
        assert float(mag.max()) < R.EXACT and torch.equal(ref, ref.float().double())
    assert 2 * p <= min(KH, KW) - 1


@pytest.mark.parametrize("ci", range(len(K.CONV_SPLITS)))
def test_split_cases_are_exact_and_split_as_stated(ci):
    name, H, W, k, p, Cin, Cout, forced, S, cps = K.CONV_SPLITS[ci]
    x, w, b, res = K.conv_exact(H, W, k, k, 1, p, Cin, Cout, "after", 40 + ci)
    _, mag = R.conv2d(x, w, b, res, 1, p, relu_after=True)
    assert float(mag.max()) < R.EXACT
    M = H * W
    per = K.CONV_B * M * Cout
    assert K.splitk(M, Cout, k * k * Cin, K.CONV_B, 16 * per, forced) == (S, cps)
    # a scratch too small for two splits: single pass
    assert K.splitk(M, Cout, k * k * Cin, K.CONV_B, 2 * per - 4, forced)[0] == 1
    starts = [s * cps for s in range(S)]
    mid = [c for c in starts if (c * 32) % Cin]
    assert len(mid) == {0: 0, 1: 2, 2: 1, 3: 3}[ci], (starts, mid)


def test_splitk_rule_on_the_gemm_case():
    # M 65, N 200: 2 x 4 tiles, K 2048 = 64 chunks -> round(800 / 8) capped at 6 <= 64 / 8
    assert K.splitk(65, 200, 2048, 1, 1 << 24) == (6, 11)
    assert K.chain_tile(2048, 6, 11) == 11 * 32 + 5
    assert K.chain_skinny(2048) == 128 + 15 and K.chain_skinny(36) == 32 + 3
    assert K.chain_skinny(256) == 32 + 7 and K.chain_skinny(8) == 8 + 3


@pytest.mark.parametrize("Kk", K.GEMM_K)
def test_exact_gemms_stay_below_2_24(Kk):
    for M in K.GEMM_M:
        A, W, b, res = K.gemm_exact(M, Kk, M * 1000 + Kk)
        ref, mag = R.gemm(A, W, b, res, relu=True)
        assert float(mag.max()) < R.EXACT
    A, W, b, aadd = K.gemm_aadd_exact(Kk, Kk)
    for from_col in (0, 64):
        ref, mag = R.gemm(A, W, b, None, aadd, from_col)
        assert float(mag.max()) < R.EXACT and 130 % 50 != 0
        assert not torch.equal(ref, R.gemm(A, W, b)[0])
    lo, _ = R.gemm(A, W, b, None, aadd, 64)
    assert torch.equal(lo[..., :64], R.gemm(A, W, b)[0][..., :64])
    assert not torch.equal(lo[..., 64:128], R.gemm(A, W, b)[0][..., 64:128])


def test_exact_stem_pool_edges_stay_below_2_24():
    for (H, W) in K.STEM_HW:
        img, w, b = K.stem_exact(H, W, H * 1000 + W)
        assert float(img.abs().max()) <= 8 and float(w.abs().max()) <= 4
        assert float(R.stem(img, w, b)[1].max()) < R.EXACT
    # the tile shapes the sizes were chosen for: Wo = 32 (one tile), 33, Ho = 5 (a cut tile row),
    # two tile columns with a ragged second
    assert [((h - 1) // 2 + 1, (w - 1) // 2 + 1) for h, w in K.STEM_HW] == \
        [(1, 1), (1, 1), (4, 5), (4, 32), (5, 33), (5, 65)]
    for S in K.EDGE_S:
        x1, w1, b1, x3, w3, b3 = K.edge_exact(S, S)
        assert float(R.mlearner_first(x1, w1, b1)[1].max()) < R.EXACT
        assert float(R.mlearner_last(x3, w3, b3)[1].max()) < R.EXACT


@pytest.mark.parametrize("m", [2, 4])
def test_exact_winograd_stays_below_2_24_through_every_stage(m):
    for (Cin, Cout) in K.WINO_CH[m]:
        for (H, W) in K.WINO_HW[m]:
            x, w, b = K.wino_exact(m, H, W, Cin, Cout, H * 16 + W)
            U = R.wino_weights(w, m)
            assert torch.equal(U, U.round()), "U must be integral after its one rounding"
            assert float((U - R.wino_weights(w, m, round_u=False)).abs().max()) < 1e-9
            out, mag, (vmax, mmax, omax) = R.wino_conv(x, w, b, m)
            assert max(vmax, mmax, omax) < R.EXACT, (m, H, W, Cin, vmax, mmax, omax)
            assert torch.equal(out, out.round())
            Mx, bias = K.wino_m_exact(m, H, W, Cout, H + W)
            assert float(R.wino_output(Mx, bias, K.WINO_B, H, W, m, absolute=True).max()) < R.EXACT


# ------------------------------------------------------------------------------ planted values
def _planted_is_zero_among_ordinary(ref, mag, idx, neighbours):
    r, g = ref[idx], mag[idx]
    assert bool((r.abs() < 1e-6 * g).all()), (r, g)
    assert bool((g > 0.1 * mag[neighbours].median()).all()), "the planted mag must be ordinary"
    near = ref[neighbours].abs()
    assert float(near.max()) > 1e3 * float(r.abs().max()) and float(near.max()) > 0.01 * float(g.min())


@pytest.mark.parametrize("ci", range(len(K.CONV_BOUNDED)))
def test_planted_convolution_values(ci):
    gi, tile, epi, kind = K.CONV_BOUNDED[ci]
    name, H, W, KH, KW, s, p, Cin, Cout = K.CONV_GEOMS[gi]
    x, w, b, res, planted = K.conv_random(H, W, KH, KW, s, p, Cin, Cout, epi, kind, 100 + ci)
    ref, mag = R.conv2d(x, w, b, res, s, p)
    assert 1.0 < float(mag.median()) < 1e5 if kind == "zero" else True
    if kind == "zero":
        py, px, co = planted
        others = [c for c in range(Cout) if c != co]
        _planted_is_zero_among_ordinary(ref, mag, (slice(None), py, px, co),
                                        (slice(None), py, px, others))
    else:
        assert H > 1 and float(x[:, 0].abs().mean()) > 1e5 * float(x[:, 1:].abs().mean())
    assert bool((ref < 0).any()) and bool((ref > 0).any())


@pytest.mark.parametrize("ci", range(len(K.GEMM_BOUNDED)))
def test_planted_gemm_values(ci):
    M, N, Kk, force, colmajor, rows, scratch = K.GEMM_BOUNDED[ci]
    A, W, b, res, aadd, (m, n) = K.gemm_random(M, N, Kk, 200 + ci, aadd_rows=rows)
    ref, mag = R.gemm(A, W, b, res, aadd)
    others = [c for c in range(N) if c != n]
    _planted_is_zero_among_ordinary(ref, mag, (0, m, n), (0, m, others))
    assert 1.0 < float(mag.median()) < 1e3


def test_planted_stem_and_winograd_values():
    for (H, W) in ((7, 9), (9, 65)):
        img, w, b, (py, px, co) = K.stem_random(H, W, "zero", H)
        ref, mag = R.conv2d(img.permute(0, 2, 3, 1), w, b, None, 2, 3)
        _planted_is_zero_among_ordinary(ref, mag, (slice(None), py, px, co),
                                        (slice(None), py, px, [c for c in range(64) if c != co]))
    for (m, H, W, Cin, Cout, relu, kind) in K.WINO_BOUNDED:
        x, w, b, planted = K.wino_random(m, H, W, Cin, Cout, kind, 300 + H * 16 + W)
        ref, _ = R.conv2d(x, w, b, None, 1, 1)
        _, mag, _ = R.wino_conv(x, w, b, m)
        if kind == "zero":
            py, px, co = planted
            assert (py, px) == (H - 1, W - 1)
            _planted_is_zero_among_ordinary(ref, mag, (slice(None), py, px, co),
                                            (slice(None), py, px, [c for c in range(Cout) if c != co]))
        else:
            assert float(x[:, 0].abs().mean()) > 1e5 * float(x[:, 1:].abs().mean())
    # the clipped last tiles the planted pixels sit in
    assert any(H % m and W % m for (m, H, W, *_r) in K.WINO_BOUNDED if _r[-1] == "zero")


# ------------------------------------------------------------------------------ the pad rule
def test_every_convolution_caller_keeps_two_pad_below_the_kernel_size():
    """pn_conv2d_nhwc_ex_f32 refuses 2 pad > min(KH, KW) - 1; the package's own calls pass
    (KH, KW, stride, pad) as literals: (3, 3, s, 1), (1, 1, s, 0) or (7, 7, 1, 3)."""
    found = 0
    pkg = os.path.join(ROOT, "pair-net_amd")
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py") or fn == "hip.py":
            continue
        src = open(os.path.join(pkg, fn)).read()
        for mt in re.finditer(r"hip\.conv2d_ex\((.*?)\)\n", src, re.S):
            args = [a.strip() for a in re.sub(r"\s+", " ", mt.group(1)).split(",")]
            nums = [a for a in args if re.fullmatch(r"\d+|stride", a)]
            geo = nums[-4:]                         # KH, KW, stride, pad close the positional list
            kh, kw, pad = int(geo[0]), int(geo[1]), int(geo[3])
            assert 2 * pad <= min(kh, kw) - 1, (fn, mt.group(1))
            found += 1
        for mt in re.finditer(r"hip\.conv2d_nhwc\((.*?)\)\n", src, re.S):
            found += 1                              # (KH == KW == 2 pad + 1 is that entry's contract)
    assert found >= 10
