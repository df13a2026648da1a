"""Inputs of tests/test_post_refs.py and tests/test_post_kernels_gpu.py, built on the host from
seeds: the shapes that reach every branch of the selection / post-processing / box-trunk kernels
and the values at which a decision goes wrong.  "Decisive" inputs live on the grid of multiples
of 1/8: two distinct candidates differ by far more than any fp32 rounding of the kernel, and ties
are exact ties, so the answer is unique under the first-index rule and is compared bit for bit."""
import math

import numpy as np
import torch

INF = math.inf
NAN = math.nan


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def grid(g, *shape, lo=-32, hi=33):
    """Multiples of 1/8 in [lo / 8, hi / 8)."""
    return torch.randint(lo, hi, shape, generator=g).float() / 8.0


# ------------------------------------------------------------------------------ softmax family
SOFT_C = [2, 3, 63, 64, 65, 128, 129, 134, 192, 193, 255, 256]
SOFT_ROWS = [1, 3, 4, 5, 9]
SOFT_KINDS = ("excluded_max", "tie_lanes", "tie_lane", "tie_ends", "neg_inf", "spread100", "grid")


def soft_row(C, kind, g, admitted=None):
    """One crafted row of C logits; the decision is among the first `admitted` columns (C - 1
    for the label kernels, C for the rest).  All values are multiples of 1/8 (or -inf)."""
    A = C - 1 if admitted is None else admitted
    x = grid(g, C, lo=-32, hi=1)                     # <= 0
    if kind == "excluded_max":                       # the largest logit sits in the last column
        x[C - 1] = 2.0
        x[int(torch.randint(0, A, (1,), generator=g))] = 1.0
    elif kind == "tie_lanes":                        # two lanes hold the maximum: the smaller wins
        a = A // 3
        b = min(A - 1, a + 1 + (A // 2))
        if (b - a) % 64 == 0 and b > a + 1:
            b -= 1
        x[a] = x[b] = 1.0
    elif kind == "tie_lane":                         # columns c and c + 64: one lane, two registers
        c = (A // 5) % 64
        if c + 64 < A:
            x[c] = x[c + 64] = 1.0
            if c + 128 < A:
                x[c + 128] = 1.0
        else:
            x[A - 1] = 1.0
    elif kind == "tie_ends":                         # first and last admitted column
        x[0] = x[A - 1] = 1.0
    elif kind == "neg_inf":
        x[torch.rand(C, generator=g) < 0.5] = -INF
        x[A // 2] = 1.0
    elif kind == "spread100":                        # the tail underflows in fp32
        x = x - 96.0
        x[(2 * A) // 3] = 4.0
    return x


def soft_input(C, rows, seed, admitted=None):
    """rows x C: row r is crafted kind (r + seed) mod 7."""
    g = gen(1000 * C + rows + seed)
    return torch.stack([soft_row(C, SOFT_KINDS[(r + seed) % 7], g, admitted) for r in range(rows)])


def soft_cases(extra_c=()):
    out = []
    for i, C in enumerate(list(extra_c) + SOFT_C):
        out.append((C, SOFT_ROWS[i % 5], i))
        if SOFT_ROWS[i % 5] != 9:
            out.append((C, 9, i + 3))              # every crafted kind at every C
    return out


def soft_random(C, rows, seed):
    return torch.randn(rows, C, generator=gen(seed)) * 3.0


SOFT_RANDOM = [(134, 400, 11), (57, 400, 12), (256, 300, 13)]       # (C, rows, seed)


def hostile_rows(C):
    """Rows whose softmax is NaN, and the admitted index torch.argmax of the logits names (0
    where no admitted logit is NaN) -> (x [n][C], expected index [n])."""
    g = gen(77 + C)
    rows, want = [], []

    def add(x, i):
        rows.append(x)
        want.append(i)
    add(torch.full((C,), -INF), 0)
    x = grid(g, C); x[C - 1] = NAN; add(x, 0)                       # only the excluded column
    x = grid(g, C); x[0] = NAN; add(x, 0)
    x = grid(g, C); x[(C - 2) // 2] = INF; add(x, 0)                # +inf: inf - inf
    if C >= 3:
        x = grid(g, C); x[C - 2] = NAN; add(x, C - 2)               # the last admitted column
        x = grid(g, C); x[1] = NAN; x[C - 2] = NAN; add(x, 1)       # the first of two
    if C - 1 > 70:
        x = grid(g, C); x[69] = NAN; x[5] = 4.0; add(x, 69)         # second register of lane 5
        x = grid(g, C); x[70] = NAN; x[6] = NAN; x[C - 1] = NAN; add(x, 6)
    return torch.stack(rows), torch.tensor(want)


# ------------------------------------------------------------------------------ row argmax
ARGMAX_N = [1, 2, 63, 64, 65, 128, 129, 1000]
ARGMAX_ROWS = [1, 5]


def argmax_input(n, rows, seed):
    g = gen(31 * n + rows + seed)
    out = []
    for r in range(rows):
        x = grid(g, n, lo=-32, hi=1)
        kind = (r + seed) % 5
        if kind == 0 and n > 1:                      # across lanes
            x[n // 3] = x[min(n - 1, n // 3 + 1)] = 1.0
        elif kind == 1 and n > 64:                   # inside a lane
            c = (n // 7) % (n - 64)
            x[c] = x[c + 64] = 1.0
        elif kind == 2:
            x[n - 1] = 1.0
        elif kind == 3:
            x[:] = -INF
        out.append(x)
    return torch.stack(out)


# ------------------------------------------------------------------------------ top-k
TOPK_N = [1, 2, 1023, 1024, 1025, 10240, 10241, 24576, 24577, 40960, 40961, 65535, 65536]
TOPK_Q = [1, 2, 32, 101, 102, 156, 157, 202, 203, 256]      # Q^2 around the same edges
TOPK_KINDS = ("equal", "two_valued", "signed_zero", "inf", "denormal", "last_bit", "kth_equal",
              "normal", "grid")


def topk_ks(n, strided=False):
    ks = [k for k in (1, 255, 256) if k <= n]
    if n <= 256:
        ks.append(n)
    if strided:
        ks += [k for k in (257, 300, 511, 512) if k <= n]
    return sorted(set(ks))


def topk_row(n, k, kind, g):
    if kind == "equal":
        return torch.full((n,), 1.5)
    if kind == "two_valued":                         # the cut falls inside the larger tie
        x = torch.full((n,), -0.25)
        m = min(n, k + 3)
        x[torch.randperm(n, generator=g)[:m]] = 0.75
        return x
    if kind == "signed_zero":
        x = torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
        x[torch.randperm(n, generator=g)[:max(1, n // 50)]] = -1.0
        return x
    if kind == "inf":
        x = grid(g, n)
        r = torch.rand(n, generator=g)
        x[r < 0.02] = INF
        x[r > 0.97] = -INF
        return x
    if kind == "denormal":                           # multiples of 2^-149, both signs, and zeros
        return torch.randint(-6, 7, (n,), generator=g).float() * 2.0 ** -149
    if kind == "last_bit":                           # neighbours one mantissa bit apart
        return 1.0 + torch.randint(0, 8, (n,), generator=g).float() * 2.0 ** -23
    x = torch.randn(n, generator=g) if kind != "grid" else grid(g, n)
    if kind == "kth_equal" and n > k:                # the k-th and the (k + 1)-th are equal
        order = torch.argsort(x, descending=True, stable=True)
        x[order[k]] = x[order[k - 1]]
    return x


def topk_input(n, k, B, seed):
    """B rows; row b is kind (b + seed) mod 9."""
    g = gen(7 * n + 13 * k + seed)
    return torch.stack([topk_row(n, k, TOPK_KINDS[(b + seed) % 9], g) for b in range(B)])


# ------------------------------------------------------------------------------ panoptic
PAN_N = [1, 2, 9]
PAN_HW = [1, 255, 256, 257, 5000]


def panoptic_input(n, HW, seed):
    """Integer-valued planes with many exact ties, labels, and a remap onto earlier planes."""
    g = gen(100 * n + HW + seed)
    masks = torch.randint(-2, 3, (n, HW), generator=g).float()
    labels = torch.randint(0, 133, (n,), generator=g)
    remap = torch.tensor([i if i % 3 else max(0, i - 3) for i in range(n)], dtype=torch.int32)
    return masks, labels, remap


def _scene(Q, h, w, NC, kept, prefs, seed=0):
    """kept: {query: (label, score)}; prefs: list of (pixel range, [queries by preference]).
    Planes: 9 / 7 / 5 for a pixel's first / second / third choice, -3 - (q mod 3) elsewhere;
    every query that must not be kept is a decoy: 20 everywhere, so keeping it shows at once."""
    HW = h * w
    g = gen(seed + Q + HW)
    labels = torch.randint(0, NC - 1, (Q,), generator=g)
    scores = torch.rand(Q, generator=g) * 0.5            # <= 0.5: not kept
    scores[::3] = 0.875
    labels[::3] = NC - 1                                  # a high score with the dropped label
    masks = torch.full((Q, HW), 20.0)
    for q, (lab, sc) in kept.items():
        labels[q], scores[q] = lab, sc
        masks[q] = -3.0 - (q % 3)
    for (p0, p1), order in prefs:
        for j, q in enumerate(order):
            masks[q, p0:p1] = 9.0 - 2.0 * j
    return dict(Q=Q, h=h, w=w, NC=NC, labels=labels, scores=scores, masks=masks.view(Q, h, w))


HALF_UP = float(np.nextafter(np.float32(0.5), np.float32(1.0)))


def pan_scenes():
    """name -> scene.  NC is the kernel's num_classes argument: label NC - 1 is dropped."""
    S = {}
    # the score threshold is strict, and the dropped label is NC - 1 alone
    S["threshold"] = _scene(5, 15, 17, 133, {1: (131, HALF_UP), 4: (133, 0.75)},
                            [((0, 100), [1, 4]), ((100, 255), [4, 1])])
    S["threshold"]["scores"][0] = 0.5                    # exactly 0.5: not kept
    S["threshold"]["labels"][0] = 3
    # 79 twice (things: apart), 80 twice (stuff: merged), areas of exactly 4 and 5, and a segment
    # that lives through round 1 on its merged area and falls out in round 2
    T1, T2, A, X, B, Y = 4, 10, 20, 31, 40, 98
    S["merge"] = _scene(100, 24, 32, 133,
                        {T1: (79, 0.9), T2: (79, 0.9), A: (80, 0.6), X: (7, 0.7), B: (80, 0.8),
                         Y: (100, 0.99)},
                        [((0, 768), [Y]), ((0, 4), [T1, Y]), ((4, 9), [T2, Y]), ((9, 12), [A, Y]),
                         ((12, 15), [B, X, Y]), ((15, 31), [X, Y])])
    S["nkeep0"] = _scene(1, 2, 2, 133, {}, [])
    S["nkeep0"]["scores"][0] = 0.25
    # four pixels: no area exceeds 4, everything is filtered
    S["all_gone"] = _scene(256, 2, 2, 133, {1: (5, 0.9), 100: (90, 0.8), 255: (90, 0.7)},
                           [((0, 2), [1, 100]), ((2, 3), [100]), ((3, 4), [255, 1])])
    S["single"] = _scene(1, 15, 17, 133, {0: (17, 0.51)}, [((0, 255), [0])])
    # exact ties between kept planes: the first kept plane wins
    S["ties"] = _scene(5, 1, 257, 91, {1: (3, 0.9), 2: (80, 0.9), 4: (80, 0.9)},
                       [((0, 200), [1]), ((50, 150), [2]), ((150, 257), [4])])
    S["ties"]["masks"][2, 0, 50:150] = 9.0
    S["ties"]["masks"][4, 0, 100:257] = 9.0
    return S


def pan_up_scene():
    """7 x 9 -> 13 x 20 with random float planes: the admissibility rule for seg."""
    g = gen(5)
    Q = 9
    labels = torch.tensor([3, 90, 132, 7, 91, 11, 45, 132, 60])
    scores = torch.tensor([0.9, 0.8, 0.9, 0.3, 0.7, 0.95, 0.5, 0.6, 0.2])
    return dict(Q=Q, h=7, w=9, ho=13, wo=20, NC=133, labels=labels, scores=scores,
                masks=torch.randn(Q, 7, 9, generator=g) * 4.0)


RESIZE_SHAPES = [(7, 9, 13, 20), (25, 42, 47, 79), (3, 5, 5, 4100)]
RESIZE_NKEEP = [0, 1, 9]

# PanState as 32-bit words: nkeep, active, rounds, all_gone, first, 11 pad, then 256 each
ST_NKEEP, ST_ACTIVE, ST_ROUNDS, ST_GONE, ST_KEPT, ST_REMAP, ST_ALIVE, ST_RANK = \
    0, 1, 2, 3, 16, 272, 528, 784


# ------------------------------------------------------------------------------ box trunk glue
def zero_rows_input(B, rows, C, ld, seed, per_image):
    g = gen(seed + rows + C)
    x = torch.randn(B, rows, ld, generator=g)
    valid = torch.rand(B if per_image else 1, rows, generator=g) < 0.6
    if rows > 1:
        valid[:, 0], valid[:, -1] = False, True
    v = valid.expand(B, rows)
    bad = torch.tensor([NAN, INF, -INF, -0.0])
    fill = bad[torch.randint(0, 4, (B, rows, ld), generator=g)]
    x = torch.where(v[..., None].expand_as(x), x, fill)          # invalid rows: NaN, +-inf, -0
    return x, valid


def box_logits(rows, seed):
    g = gen(seed + rows)
    x = torch.randn(rows, 4, generator=g) * 3.0
    special = torch.tensor([0.0, 20.0, -20.0, INF, -INF, -0.0, 88.0, -88.0])
    flat = x.view(-1)
    n = min(flat.numel(), 8)
    flat[torch.randperm(flat.numel(), generator=g)[:n]] = special[:n]
    return x


REFINE_REF = [-0.1, 0.0, 1e-6, 1e-5, 0.5, 1.0 - 1e-5, 1.0, 1.2]
REFINE_DELTA = [0.0, 5.0, -5.0, INF, -INF]


def refine_input(rows, seed):
    """Every (ref_in, delta) pair of the two lists, then random ones, over rows * 4 elements."""
    g = gen(seed + rows)
    n = rows * 4
    ref = torch.rand(n, generator=g)
    delta = torch.randn(n, generator=g) * 2.0
    pairs = [(r, d) for r in REFINE_REF for d in REFINE_DELTA]
    start = (seed * 7) % len(pairs)
    for i in range(min(n, len(pairs))):
        r, d = pairs[(start + i) % len(pairs)]
        ref[i], delta[i] = r, d
    return delta.view(rows, 4), ref.view(rows, 4)


def sampling_logits(g, rows, NP):
    """[rows][8][NP]: per (row, head) one of equal / one dominant by 80 / some -inf / wide."""
    lg = torch.randn(rows, 8, NP, generator=g)
    kind = torch.arange(rows * 8).view(rows, 8) % 4
    lg[kind == 0] = 0.375
    dom = lg[kind == 1]
    dom[:, 0] += 80.0
    lg[kind == 1] = dom
    ninf = lg[kind == 2]
    if NP > 1:
        ninf[:, 1::2] = -INF
    lg[kind == 2] = ninf
    lg[kind == 3] = lg[kind == 3] * 20.0
    return lg


def box_sampling_input(B, rpi, L, ld_extra, seed):
    g = gen(seed + 10 * L + rpi)
    rows, NP = B * rpi, L * 4
    ld = 8 * NP * 3 + ld_extra
    offaw = torch.full((rows, ld), NAN)
    offaw[:, :8 * NP * 2] = torch.randn(rows, 8 * NP * 2, generator=g) * 2.0
    offaw[:, 8 * NP * 2:8 * NP * 3] = sampling_logits(g, rows, NP).view(rows, -1)
    ref = torch.rand(rows, 4, generator=g)
    vr = 0.5 + 0.5 * torch.rand(B, L, 2, generator=g)            # per image, level and axis
    return offaw, ref, vr


TOKEN_SHAPES = {1: [(3, 5)], 2: [(3, 5), (2, 3)], 3: [(5, 7), (3, 4), (2, 2)],
                4: [(6, 9), (3, 5), (2, 3), (1, 2)]}


def token_sampling_input(L, B, ld_extra, seed):
    g = gen(seed + L)
    shapes = TOKEN_SHAPES[L]
    N, NP = sum(h * w for h, w in shapes), L * 4
    ld = 8 * NP * 3 + ld_extra
    offaw = torch.full((B, N, ld), NAN)
    offaw[..., :8 * NP * 2] = torch.randn(B, N, 8 * NP * 2, generator=g)
    offaw[..., 8 * NP * 2:8 * NP * 3] = sampling_logits(g, B * N, NP).view(B, N, -1)
    vr = 0.4 + 0.6 * torch.rand(B, L, 2, generator=g)
    return offaw, vr, shapes


def level_edges(shapes):
    """Token indices of the first and the last token of every level."""
    out, s = [], 0
    for h, w in shapes:
        out += [s, s + h * w - 1]
        s += h * w
    return out


QS_B, QS_NQ, QS_C = [1, 2], [1, 3, 4, 5, 300], [1, 63, 64, 65, 133, 256]


def query_score_input(B, Nq, C, seed):
    return torch.randn(B, Nq, C, generator=gen(seed + Nq + C)) * 3.0


TRIP_R, TRIP_C = [1, 2, 3, 100], [2, 64, 65, 134]
TRIP_SF = [1.5, 1.25, 2.0, 0.75]                  # four distinct scale factors


def box_triplets_input(R, C, seed):
    """Grid logits with ties across and inside lanes; boxes leaving each of the four edges,
    zero-size boxes, ordinary ones."""
    g = gen(seed + 10 * R + C)
    cls = [soft_input(C, R, seed + s, admitted=C) for s in (0, 3)]
    boxes = []
    crafted = torch.tensor([[0.05, 0.5, 0.3, 0.2],     # leaves the left edge
                            [0.5, 0.04, 0.2, 0.3],     # the top
                            [0.95, 0.5, 0.3, 0.2],     # the right
                            [0.5, 0.97, 0.2, 0.3],     # the bottom
                            [0.4, 0.6, 0.0, 0.0],      # zero size
                            [0.5, 0.5, 1.5, 1.5]])     # all four
    for s in range(2):
        b = torch.rand(R, 4, generator=g) * torch.tensor([1.0, 1.0, 0.5, 0.5])
        for r in range(R):
            if r < 6 or r % 2 == 0:
                b[r] = crafted[(r + 3 * s + seed) % 6]
        boxes.append(b)
    return cls[0], cls[1], boxes[0], boxes[1]


SINE_HW = [(1, 1), (3, 5), (13, 21)]
SINE_C = [4, 8, 256]


def sine_valids(h, w):
    """full, (h, w - 2), (h - 1, w), (2, 3), clipped into the map."""
    out = []
    for vh, vw in ((h, w), (h, w - 2), (h - 1, w), (2, 3)):
        v = (max(1, min(vh, h)), max(1, min(vw, w)))
        if v not in out:
            out.append(v)
    return out
