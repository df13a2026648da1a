"""Every input of tests/test_mm_kernels_gpu.py (but the zero operands of its refused calls), built
on the host from seeded generators so that tests/test_mm_refs.py can check, without a GPU, every
condition the GPU file relies on: the integer cases stay below 2^24 through every intermediate,
the planted pixels really cancel, the split-K rule restated here gives the split counts written
beside the cases.  Nothing here calls a kernel."""
import torch

GEMM_GROUP_MAX = 18


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------ the library's rules
def cdiv(a, b):
    return -(-a // b)


def splitk(M, N, K, batch, scratch_floats, forced=0):
    """(splits, chunks per split) of the 64x64 tile path: splitk_factor() of csrc/gemm.hip for an
    aligned scratch and bias and N % 4 == 0."""
    nk, tiles = cdiv(K, 32), cdiv(M, 64) * cdiv(N, 64) * batch
    if scratch_floats <= 0 or N % 4 or forced == 1:
        return 1, nk
    if not forced and (tiles >= 1024 or nk < 8):
        return 1, nk
    S = forced if forced else (1600 + tiles) // (2 * tiles)
    if not forced:
        S = min(S, 6, nk // (16 if tiles > 400 else 8))
    S = min(S, 16, nk)
    per = batch * M * N
    if S * per > scratch_floats:
        S = scratch_floats // per
    if S < 2:
        return 1, nk
    cps = cdiv(nk, S)
    return cdiv(nk, cps), cps


def skinny_waves(K):
    """K slices (waves) of a k_gemm_skinny workgroup: launch_skinny() of csrc/gemm.hip."""
    return 4 if K <= 128 else 8 if K <= 256 else 16


def chain_tile(K, splits=1, cps=None):
    """Roundings of a tile kernel's contraction: one per k of the fmaf chain (the MFMA's two
    products are two steps of it); split-K: the longest slice's chain and the reduce's S - 1 adds
    in slice order."""
    return K if splits <= 1 else min(32 * cps, K) + splits - 1


def chain_skinny(K):
    """k_gemm_skinny: wave w contracts a slice of ceil(K / NW) rounded up to 32, then NW - 1 adds
    in wave order."""
    nw = skinny_waves(K)
    ks = (cdiv(K, nw) + 31) & ~31
    return min(ks, K) + nw - 1


def chain_gemm(K, force):
    return chain_skinny(K) if force == "skinny" or K < 32 else chain_tile(K)


# ------------------------------------------------------------------------------ convolution
# (name, H, W, KH, KW, stride, pad, Cin, Cout): the geometries of the issue; across them Cin in
# {32, 64, 96} and Cout in {32, 64, 96, 200}
CONV_GEOMS = [
    ("1x1 image, eight taps outside", 1, 1, 3, 3, 1, 1, 32, 32),
    ("image smaller than the kernel", 2, 3, 7, 7, 1, 3, 32, 64),
    ("stride 2, 5x6", 5, 6, 3, 3, 2, 1, 64, 96),
    ("stride 2, 6x5", 6, 5, 3, 3, 2, 1, 96, 32),
    ("1x1 stride 2", 5, 6, 1, 1, 2, 0, 96, 200),
    ("M = 64", 8, 8, 3, 3, 1, 1, 64, 64),
    ("M = 65", 5, 13, 3, 3, 1, 1, 32, 200),
    ("3x5 taps", 9, 7, 3, 5, 1, 1, 64, 32),
    ("5x3 taps", 9, 7, 5, 3, 1, 1, 32, 96),
    ("valid convolution", 4, 5, 3, 3, 1, 0, 96, 64),
]
CONV_TILES = [None, "128x64", "128"]
EPILOGUES = ["relu", "res", "after"]      # ReLU; residual; residual then ReLU
CONV_B = 2

# Split-K, scratch supplied.  (name, H, W, K, pad, Cin, Cout, forced, splits, chunks per split):
# chunk c of a 3x3 / 7x7 kernel with Cin = 64 is the half ci0 = 32 (c % 2) of tap c / 2, so a split
# that starts at an odd chunk starts in the middle of a tap.
CONV_SPLITS = [
    # 9 chunks = 9 taps, 3 per split: splits start at chunks 0, 3, 6 = taps 0, 3, 6 (on taps)
    ("Cin 32 3x3 KSPLIT(3)", 8, 8, 3, 1, 32, 64, 3, 3, 3),
    # 18 chunks, ceil(18 / 4) = 5 per split, 4 splits: starts at chunks 0, 5, 10, 15 = tap 2 second
    # half (mid-tap), tap 5 (on it), tap 7 second half (mid-tap)
    ("Cin 64 3x3 KSPLIT(4)", 5, 13, 3, 1, 64, 64, 4, 4, 5),
    # the rule: 4 tiles -> round(800 / 4) capped at 6, then at 18 / 8 = 2 splits of 9 chunks: the
    # second starts at chunk 9 = tap 4 second half (mid-tap)
    ("Cin 64 3x3 rule", 5, 13, 3, 1, 64, 64, 0, 2, 9),
    # 98 chunks, 4 tiles -> 6 splits (98 / 8 = 12 allows them) of ceil(98 / 6) = 17 (the last: 13):
    # starts at chunks 0, 17, 34, 51, 68, 85 = tap 8 second half (mid), tap 17 (on), tap 25 second
    # half (mid), tap 34 (on), tap 42 second half (mid)
    ("Cin 64 7x7 rule", 5, 13, 7, 3, 64, 64, 0, 6, 17),
]


def epilogue_kw(epi):
    return dict(relu=epi == "relu", relu_after=epi == "after")


def conv_out(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def pack_conv_weight(w):
    """torch's [Cout][Cin][KH][KW] -> Wp [Cout][(ky KW + kx) Cin + ci]."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def conv_exact(H, W, KH, KW, stride, pad, Cin, Cout, epi, seed):
    """Integer operands in [-8, 8] -> (x [B][H][W][Cin], w [Cout][Cin][KH][KW], bias, res|None)."""
    g = gen(seed)
    Ho, Wo = conv_out(H, W, KH, KW, stride, pad)
    x, w = ints(g, -8, 8, CONV_B, H, W, Cin), ints(g, -8, 8, Cout, Cin, KH, KW)
    bias = ints(g, -8, 8, Cout)
    res = ints(g, -8, 8, CONV_B, Ho, Wo, Cout) if epi != "relu" else None
    return x, w, bias, res


def plant_window(x, w, py, px, stride, pad, co):
    """Makes output (py, px, co) of the convolution a sum of exactly cancelling pairs: inside its
    window the odd input channels are minus the even ones, and output channel co weighs both
    members of a pair alike."""
    KH, KW = w.shape[2], w.shape[3]
    H, W_ = x.shape[1], x.shape[2]
    for ky in range(KH):
        for kx in range(KW):
            iy, ix = py * stride + ky - pad, px * stride + kx - pad
            if 0 <= iy < H and 0 <= ix < W_:
                x[:, iy, ix, 1::2] = -x[:, iy, ix, 0::2]
    w[co, 1::2] = w[co, 0::2]


def wscale(K):
    """Weight scale that keeps mag = sum |x| |w| of a K-term contraction of randn(scale 2) inputs
    at order 1 .. 100."""
    return 0.5 * min(1.0, 128.0 / K)


def conv_random(H, W, KH, KW, stride, pad, Cin, Cout, epi, kind, seed):
    """Random operands with mag of order 1 .. 100 -> (x, w, bias, res|None, planted).
    kind "zero": output (py, px, co) = planted is a sum of cancelling pairs (bias and residual 0
    there) among ordinary neighbours; kind "border": image row 0 has magnitude 1e3, the interior
    1e-3 (planted = None)."""
    g = gen(seed)
    Ho, Wo = conv_out(H, W, KH, KW, stride, pad)
    x = randn(g, CONV_B, H, W, Cin, scale=2.0)
    w = randn(g, Cout, Cin, KH, KW, scale=wscale(Cin * min(KH, H) * min(KW, W)))
    bias = randn(g, Cout)
    res = randn(g, CONV_B, Ho, Wo, Cout, scale=3.0) if epi != "relu" else None
    planted = None
    if kind == "zero":
        planted = (Ho // 2, Wo // 2, Cout // 3)
        plant_window(x, w, planted[0], planted[1], stride, pad, planted[2])
        bias[planted[2]] = 0.0
        if res is not None:
            res[:, planted[0], planted[1], planted[2]] = 0.0
    else:
        x[:, 0] *= 1e3
        x[:, 1:] *= 1e-3
    return x, w, bias, res, planted


# (geometry index, tile, epilogue, kind): the smallest member per branch of the exact geometries
CONV_BOUNDED = [
    (0, None, "relu", "zero"), (1, None, "res", "zero"), (2, None, "after", "border"),
    (3, None, "relu", "zero"), (4, None, "res", "zero"), (4, None, "after", "border"),
    (5, "128x64", "relu", "zero"), (5, "128", "res", "border"), (6, None, "after", "zero"),
    (6, None, "relu", "border"), (7, None, "res", "zero"), (8, None, "after", "border"),
    (9, None, "relu", "zero"), (6, "128x64", "res", "border"), (6, "128", "after", "zero"),
]
# the 1x1 convolution of the issue's "L ~ 34" (Cin = 32: 32 + bias + residual) and the long chain
CONV_BOUNDED_EXTRA = [
    ("1x1 Cin 32", 5, 6, 1, 1, 1, 0, 32, 64),
    ("7x7 Cin 64 (K = 3136)", 5, 13, 7, 7, 1, 3, 64, 64),
]


# ------------------------------------------------------------------------------ dense contraction
GEMM_M = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 132]
GEMM_N = 200
GEMM_K = [8, 28, 36, 96, 260]
GEMM_FORMS = ["tile", "tile128x64", "skinny"]        # the forms test_gemm_ragged_edges leaves out


def gemm_exact(M, K, seed, batch=2, N=GEMM_N):
    """Integer operands -> (A [Z][M][K], W [Z][N][K], bias [N], res [Z][M][N])."""
    g = gen(seed)
    return (ints(g, -8, 8, batch, M, K), ints(g, -8, 8, batch, N, K), ints(g, -8, 8, N),
            ints(g, -8, 8, batch, M, N))


def gemm_aadd_exact(K, seed, M=130, rows=50, N=GEMM_N):
    g = gen(seed)
    return (ints(g, -8, 8, 1, M, K), ints(g, -8, 8, 1, N, K), ints(g, -8, 8, N),
            ints(g, -8, 8, rows, K))


def gemm_random(M, N, K, seed, batch=1, aadd_rows=0):
    """Random operands -> (A, W, bias, res, aadd|None, planted): C[0][m][n] at planted = (m, n) is
    a sum of cancelling pairs (A[m] odd columns = minus the even ones, W[n] pairs alike, bias and
    residual 0 there; with an addend its rows m % rows carry the same pairing)."""
    g = gen(seed)
    A, W_ = randn(g, batch, M, K, scale=2.0), randn(g, batch, N, K, scale=wscale(K))
    bias, res = randn(g, N), randn(g, batch, M, N, scale=3.0)
    aadd = randn(g, aadd_rows, K) if aadd_rows else None
    m, n = M // 2, (N * 2) // 3
    A[:, m, 1::2] = -A[:, m, 0::2]
    W_[:, n, 1::2] = W_[:, n, 0::2]
    if aadd is not None:
        aadd[m % aadd_rows, 1::2] = -aadd[m % aadd_rows, 0::2]
    bias[n] = 0.0
    res[:, m, n] = 0.0
    return A, W_, bias, res, aadd, (m, n)


# (M, N, K, force, colmajor, aadd rows, scratch): K in {32, 36, 256} under every form, and the
# production depth K = 2048 through split-K (8 tiles -> 6 splits of ceil(64 / 6) = 11 chunks)
GEMM_BOUNDED = [(65, 200, K, f, False, 0, False) for K in (32, 36, 256)
                for f in ("tile", "tile128x64", "tile64", "skinny")] + \
    [(65, 200, 36, "tile64", True, 0, False), (64, 200, 36, "tile", True, 0, False),
     (130, 200, 36, "tile64", False, 50, False), (130, 200, 256, "skinny", False, 50, False),
     (65, 200, 2048, "tile64", False, 0, True), (65, 200, 2048, "skinny", False, 0, False)]


# ------------------------------------------------------------------------------ stem, pool, edges
STEM_HW = [(1, 1), (2, 2), (7, 9), (8, 64), (9, 65), (10, 130)]
STEM_B = 2


def pack_stem_weight(w):
    """[64][3][7][7] -> Wp [64][160]: k = c 49 + ky 7 + kx, zero-padded from 147."""
    wp = torch.zeros(64, 160)
    wp[:, :147] = w.reshape(64, 147)
    return wp


def stem_exact(H, W, seed):
    g = gen(seed)
    return ints(g, -8, 8, STEM_B, 3, H, W), ints(g, -4, 4, 64, 3, 7, 7), ints(g, -8, 8, 64)


def stem_random(H, W, kind, seed):
    """kind "zero": output (py, px, co): inside its window image channel 1 = minus channel 0 and
    channel 2 = 0, channel co weighs channels 0 and 1 alike and its bias is 0; "border": row 0 of
    the image 1e3, the rest 1e-3."""
    g = gen(seed)
    img, w, bias = randn(g, STEM_B, 3, H, W, scale=2.0), randn(g, 64, 3, 7, 7, scale=0.5), randn(g, 64)
    planted = None
    if kind == "zero":
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        planted = (Ho // 2, Wo // 2, 21)
        y0, x0 = max(2 * planted[0] - 3, 0), max(2 * planted[1] - 3, 0)
        y1, x1 = min(2 * planted[0] + 4, H), min(2 * planted[1] + 4, W)
        img[:, 1, y0:y1, x0:x1] = -img[:, 0, y0:y1, x0:x1]
        img[:, 2, y0:y1, x0:x1] = 0.0
        w[21, 1] = w[21, 0]
        bias[21] = 0.0
    else:
        img[:, :, 0] *= 1e3
        img[:, :, 1:] *= 1e-3
    return img, w, bias, planted


POOL_SIDES = [1, 2, 3, 4, 5]
POOL_C = [4, 64]
POOL_KINDS = ["negative", "neginf", "ordinary"]


def pool_input(H, W, C, kind, seed):
    g = gen(seed)
    x = randn(g, 2, H, W, C)
    if kind != "ordinary":
        x = -x.abs() - 0.5                 # all negative: a padding of 0 would win every border
    if kind == "neginf":
        x[0, 0, 0, :] = float("-inf")      # a window of -inf alone (H = W = 1), or one among finite
        x[1, H - 1, W - 1, C // 2] = float("-inf")
    return x


EDGE_S = [1, 5, 8, 9, 17]


def edge_exact(S, seed):
    """-> (x1 [B][S][S], w1 [64][49], b1 [64], x3 [B][S][S][64], w3 [49][64], b3 [1])."""
    g = gen(seed)
    return (ints(g, -8, 8, 2, S, S), ints(g, -8, 8, 64, 49), ints(g, -8, 8, 64),
            ints(g, -8, 8, 2, S, S, 64), ints(g, -8, 8, 49, 64), ints(g, -8, 8, 1))


def edge_random(S, seed):
    g = gen(seed)
    return (randn(g, 2, S, S, scale=2.0), randn(g, 64, 49, scale=0.5), randn(g, 64),
            randn(g, 2, S, S, 64, scale=2.0), randn(g, 49, 64, scale=0.5), randn(g, 1))


# ------------------------------------------------------------------------------ Winograd
WINO_HW = {2: [(2, 2), (2, 3), (3, 2), (4, 4), (5, 7)],
           4: [(1, 1), (1, 5), (3, 5), (4, 4), (5, 9), (7, 10), (8, 12)]}
WINO_CH = {2: [(4, 4), (32, 64)], 4: [(4, 4), (32, 32)]}
WINO_B = 2


def wino_exact(m, H, W, Cin, Cout, seed):
    """F(2x2, 3x3): weights multiples of 4 (G holds halves: U = G g G^T is integral), inputs in
    [-8, 8].  F(4x4, 3x3): weights in {-576, 0, 576} (G holds 24ths), inputs in {-1, 0, 1}.
    -> (x [B][H][W][Cin], w [Cout][Cin][3][3], bias)."""
    g = gen(seed)
    if m == 2:
        return (ints(g, -8, 8, WINO_B, H, W, Cin), 4.0 * ints(g, -2, 2, Cout, Cin, 3, 3),
                ints(g, -8, 8, Cout))
    return (ints(g, -1, 1, WINO_B, H, W, Cin), 576.0 * ints(g, -1, 1, Cout, Cin, 3, 3),
            ints(g, -8, 8, Cout))


def wino_m_exact(m, H, W, C, seed):
    """An integer M [(m + 2)^2][T][C] for the output transform alone (|A|^T |M| |A| <= 19^2 64)."""
    g = gen(seed)
    th, tw = (H + m - 1) // m, (W + m - 1) // m
    return ints(g, -64, 64, (m + 2) ** 2, WINO_B * th * tw, C), ints(g, -8, 8, C)


def wino_random(m, H, W, Cin, Cout, kind, seed):
    """As conv_random for the 3x3 pad-1 convolution; the planted pixel is the last one,
    (H - 1, W - 1), in the clipped last tile when H, W are no multiples of m."""
    g = gen(seed)
    x, w, bias = randn(g, WINO_B, H, W, Cin, scale=2.0), randn(g, Cout, Cin, 3, 3, scale=0.5), randn(g, Cout)
    planted = None
    if kind == "zero":
        planted = (H - 1, W - 1, Cout // 3)
        plant_window(x, w, H - 1, W - 1, 1, 1, planted[2])
        bias[planted[2]] = 0.0
    else:
        x[:, 0] *= 1e3
        x[:, 1:] *= 1e-3
    return x, w, bias, planted


# (m, H, W, Cin, Cout, relu, kind)
WINO_BOUNDED = [(2, 5, 7, 32, 64, False, "zero"), (2, 5, 7, 32, 64, True, "border"),
                (2, 2, 3, 4, 4, False, "zero"), (4, 5, 9, 32, 32, False, "zero"),
                (4, 7, 10, 32, 32, True, "border"), (4, 7, 10, 32, 32, False, "zero"),
                (4, 1, 5, 4, 4, False, "zero"), (4, 3, 5, 4, 4, False, "border")]
