"""Every input of tests/test_fwd_kernels_gpu.py (but the zero operands of its refused calls),
built on the host from seeded generators so that tests/test_fwd_refs.py can check, without a GPU,
every condition the GPU file states about them
(planted rows really have the property they are named for; the caps on left-out elements hold
from the float64 reference alone).  Nothing here calls a kernel."""
import itertools

import torch

ATT_SMALL_MAX, ATT_WANT_WGS, ATT_MAXCH, ATT_MIN_CHUNK = 512, 512, 256, 64   # csrc/attn.hip


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------ attention
def attn_chunking(Nk, B, Q):
    """(chunk, nchunks) of the long-key path: attn_chunking() of csrc/attn.hip."""
    want = min(max(ATT_WANT_WGS // (8 * B * ((Q + 127) // 128)), 1), ATT_MAXCH)
    ch = max(((Nk + want - 1) // want + 31) & ~31, ATT_MIN_CHUNK)
    return ch, (Nk + ch - 1) // ch


def attn_waves(Nk):
    """Waves that split the keys of a k_attn_small workgroup (4 up to 4 tiles, else 8)."""
    return 4 if (Nk + 31) // 32 <= 4 else 8


ATT_BQ = [(1, 1), (2, 31), (1, 33), (2, 100)]
ATT_NK = [1, 31, 32, 33, 128, 129, 512, 513, 577, 1100]
# (B, Q, Nk, masked, kind); kind "big": scores of magnitude ~300 in natural units (q scaled);
# (33, 1, 513): B * ceil(Q / 128) = 33 > 32 workgroup rows leave attn_chunking one chunk, so
# k_attn_chunk writes the final rows itself
ATT_CASES = [(B, Q, Nk, m, "plain") for Nk in ATT_NK for (B, Q) in ATT_BQ for m in (False, True)] + \
    [(33, 1, 513, False, "plain"), (33, 1, 513, True, "plain"),
     (2, 33, 129, False, "big"), (2, 33, 129, True, "big"),
     (2, 33, 577, False, "big"), (2, 33, 577, True, "big")]

MASK_KINDS = ["all", "only0", "onlylast", "tile", "wave", "chunk"]


def mask_logits(B, Q, Nk, seed):
    """Mask logits [B*Q][Nk] (negative = masked) with planted rows -> (logits, {kind: row}).
      all       every key masked (`rowall` un-masks the row)
      only0     key 0 alone is live
      onlylast  key Nk - 1 alone is live (in the ragged last tile)
      tile      one whole 32-key tile is dead, the rest live
      wave      every tile of one wave's share is dead (k_attn_small: tiles 1, 1 + NW, ...), the
                rest live
      chunk     long path: one whole chunk is dead, the rest live
      block     long path, Q >= 64: queries 32..63 of image 0 (one wave of k_attn_chunk) all have
                keys 64..95 dead, so the wave skips that tile (`__all(dead == ~0)`); the rows are
                otherwise random and carry no other planted kind
    Kinds that need more keys than the case has are not planted; with fewer rows than kinds the
    planted ones rotate with Nk."""
    g = gen(seed)
    R = B * Q
    x = torch.rand(R, Nk, generator=g) * 2.0 - 1.0
    x[x == 0] = 0.5
    ntiles = (Nk + 31) // 32
    kinds = ["all", "only0", "onlylast"]
    if ntiles >= 2:
        kinds.append("tile")
    if Nk <= ATT_SMALL_MAX and ntiles >= 3:
        kinds.append("wave")
    if Nk > ATT_SMALL_MAX and attn_chunking(Nk, B, Q)[1] >= 2:
        kinds.append("chunk")
    kinds = kinds[Nk % len(kinds):] + kinds[:Nk % len(kinds)]
    planted = {}
    for i, kind in enumerate(kinds[:R] if R < len(kinds) else kinds):
        r = (i * 7 + 3) % R if R >= len(kinds) * 7 else i % R
        if kind == "all":
            x[r] = -x[r].abs()
        elif kind == "only0":
            x[r] = -1.0
            x[r, 0] = 1.0
        elif kind == "onlylast":
            x[r] = -1.0
            x[r, Nk - 1] = 1.0
        elif kind == "tile":
            x[r] = x[r].abs()
            x[r, 32:64] = -1.0
        elif kind == "wave":
            x[r] = x[r].abs()
            for t in range(1, ntiles, attn_waves(Nk)):
                x[r, 32 * t:32 * t + 32] = -1.0
        elif kind == "chunk":
            ch = attn_chunking(Nk, B, Q)[0]
            x[r] = x[r].abs()
            x[r, ch:2 * ch] = -1.0
        planted[kind] = r
    if Nk > ATT_SMALL_MAX and Q >= 64:
        assert not [r for r in planted.values() if 32 <= r < 64]
        x[32:64, 64:96] = -1.0
        planted["block"] = 32
    return x, planted


def attn_packed_inputs(B, Q, seed):
    """Self-attention operands as the decoder packs them: [Q | K] rows [B*Q][512], V [B*Q][256]."""
    g = gen(seed)
    return torch.randn(B * Q, 512, generator=g), torch.randn(B * Q, 256, generator=g)


def attn_inputs(B, Q, Nk, kind, seed):
    g = gen(seed)
    q = torch.randn(B, Q, 256, generator=g)
    k = torch.rand(B, Nk, 256, generator=g) * 2.0 - 1.0
    v = torch.randn(B, Nk, 256, generator=g)
    if kind == "big":
        q = q * 170.0       # scale q . k has a standard deviation of ~100: the row maximum ~300
    return q, k, v


# ------------------------------------------------------------------------------ window attention
def window_cases():
    out = []
    for i, (ws, sh, m) in enumerate(itertools.product((4, 7, 12), (0, 1), range(3))):
        H, W = [(ws, ws), (ws + 1, 2 * ws - 1), (ws - 1, ws - 2)][m]
        out.append((2, H, W, 3 if i % 2 else 1, ws, (ws // 2) * sh, False))
    out.append((2, 8, 13, 3, 7, 3, True))      # bias-table entries of +-30
    return out


def window_module(B, H, W, heads, ws, shift, big_bias, seed):
    """oracle.swin.ShiftWindowMSA (fp32, identity output projection) with seeded weights and
    tokens x [B][H*W][C]: the kernel's qkv rows are the module's own `w_msa.qkv(x)`, the fp32
    oracle is the module itself.  big_bias: bias-table entries of +-30."""
    from oracle.swin import ShiftWindowMSA
    g = gen(seed)
    C = heads * 32
    m = ShiftWindowMSA(C, heads, ws, shift)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    if big_bias:
        table[::5] = 30.0
        table[2::7] = -30.0
    m.w_msa.relative_position_bias_table.data = table
    m.w_msa.qkv.weight.data = torch.randn(3 * C, C, generator=g) * C ** -0.5
    m.w_msa.qkv.bias.data = torch.randn(3 * C, generator=g)
    m.w_msa.proj.weight.data, m.w_msa.proj.bias.data = torch.eye(C), torch.zeros(C)
    return m.eval(), torch.randn(B, H * W, C, generator=g)


# ------------------------------------------------------------------------------ normalisations
ROW_KINDS = ["benign", "offset", "constant", "tiny", "huge"]


def norm_rows(rows, C, seed, const=None):
    """[rows][C] with row i of kind ROW_KINDS[(i + rows) % 5]: benign N(0.7, 3); 1000 + 0.01
    noise; constant; magnitude 1e-20; magnitude 1e15 -> (x, kinds)."""
    g = gen(seed)
    x = torch.randn(rows, C, generator=g) * 3.0 + 0.7
    kinds = [ROW_KINDS[(i + rows) % 5] for i in range(rows)]
    for i, kd in enumerate(kinds):
        n = torch.randn(C, generator=g)
        if kd == "offset":
            x[i] = 1000.0 + 0.01 * n
        elif kd == "constant":
            x[i] = const if const is not None else float(torch.randn((), generator=g)) * 7.3
        elif kd == "tiny":
            x[i] = 1e-20 * n
        elif kd == "huge":
            x[i] = 1e15 * n
    return x, kinds


def norm_affine(C, seed):
    """gamma with entries of 1e-4 and of 0, beta."""
    g = gen(seed)
    gamma, beta = torch.randn(C, generator=g) + 1.0, torch.randn(C, generator=g)
    gamma[0], gamma[C // 2], gamma[C - 1] = 1e-4, 0.0, 1e-4
    return gamma, beta


def groupnorm_input(B, HW, seed):
    """[B][HW][256], G = 32: group 0 has mean 1e3 and spread 1e-2, group 1 is constant."""
    g = gen(seed)
    x = torch.randn(B, HW, 256, generator=g) * 2.0 + 2.0
    x[:, :, 0:8] = 1000.0 + 0.01 * torch.randn(B, HW, 8, generator=g)
    x[:, :, 8:16] = -2.7182817459106445
    return x


L2_KINDS = ["zero", "below_eps", "small", "huge", "onehot", "benign"]


def l2_rows(rows, seed):
    g = gen(seed)
    x = torch.randn(rows, 256, generator=g)
    kinds = [L2_KINDS[i % 6] for i in range(rows)]
    for i, kd in enumerate(kinds):
        unit = x[i] / x[i].norm()
        if kd == "zero":
            x[i] = 0.0
        elif kd == "below_eps":
            x[i] = unit * 1e-13
        elif kd == "small":
            x[i] = unit * 1e-6
        elif kd == "huge":
            x[i] = unit * 1e15
        elif kd == "onehot":
            x[i] = 0.0
            x[i, (37 * i) % 256] = -3.7 if i % 2 else 1.9e-3
    return x, kinds


def gelu_input(n, seed):
    """+-10, +-1e-8, 0, the range where erf saturates (|x| / sqrt 2 in 3 .. 6), and N(0, 2)."""
    special = torch.tensor([10.0, -10.0, 1e-8, -1e-8, 0.0, -0.0, 4.3, -4.3, 5.5, -5.5, 6.1, -6.1,
                            8.4, -8.4, -3.9, 3.9])
    x = torch.randn(n, generator=gen(seed)) * 2.0
    m = min(n, len(special))
    x[:m] = special[(torch.arange(m) + n) % len(special)]
    return x


def patch_merge_input(B, H, W, C, seed):
    return torch.randn(B, H * W, C, generator=gen(seed)) * 3.0 + 0.7


# ------------------------------------------------------------------------------ samplers
BIL_L = 5           # l0 = 1 - l1; l0x v00, + l1x v01, x l0y, + the other row
BIL_COORD = 3       # src = scale (dst + 0.5) - 0.5: the quotient, the product, the difference


def bilinear_extra(hi, wi, spread):
    """The coordinate term of a resize, both axes: BIL_COORD roundings of at most 2^-24 (1 + in)
    of a pixel, times the taps' largest difference (fwd_ref.bilinear's spread)."""
    return BIL_COORD * (2.0 + hi + wi) * spread


def bilinear_input(B, C, hi, wi, ho, wo):
    """Planes [B][C][hi][wi] of N(0, 4) and the base [B][ho*wo][C] the accumulating form adds to."""
    g = gen(hi * wi + ho)
    return torch.randn(B, C, hi, wi, generator=g) * 4.0, torch.randn(B, ho * wo, C, generator=g)


def upadd_coarse(B, hc, wc, seed):
    return torch.randn(B, hc * wc, 256, generator=gen(seed)) * 2.0


BILINEAR_SIZES = [(1, 1, 3, 5), (3, 5, 1, 1), (2, 3, 7, 8), (2, 3, 7, 9), (40, 67, 5, 9),
                  (5, 7, 5, 7)]

MSDA_SHAPES = [[(1, 1)], [(3, 5)], [(1, 5), (4, 2)], [(2, 4), (1, 1), (3, 5), (5, 1)]]   # odd N


def msda_value(B, shapes, seed):
    n = sum(h * w for h, w in shapes)
    return torch.randn(B, n, 8, 32, generator=gen(seed))


def planted_pixels(h, w):
    """Pixel coordinates (x, y) the planted taps aim at, per sampling point 0..3 and variant
    0..3: a pixel centre; exactly -0.5; the far edges w - 0.5 / h - 0.5; one pixel outside and
    1e4 pixels outside."""
    return [[(w // 2, h // 2), (0.0, h - 1.0), (w - 1.0, 0.0), (w // 2, 0.0)],
            [(-0.5, h // 2), (w // 2, -0.5), (-0.5, -0.5), (-0.5, h - 0.5)],
            [(w - 0.5, h // 2), (w // 2, h - 0.5), (w - 0.5, h - 0.5), (w - 0.5, -0.5)],
            [(-1.0, h // 2), (w // 2, float(h)), (-1e4, h // 2), (w // 2, 1e4)]]


def msda_offsets(B, shapes, seed, spread_logits=False):
    """Encoder-form inputs: offsets [B][N][8][L][4][2] (pixels) and logits [B][N][8][L*4].
    Heads 0..3 of every token carry the planted taps (variant = head) at every level: the
    offset is the planted pixel minus the token's own position at that level, (qx + 0.5) / qw *
    w_l - 0.5, rounded to fp32; heads 4..7 are N(0, 3 px)."""
    g = gen(seed)
    L = len(shapes)
    n = sum(h * w for h, w in shapes)
    off = torch.randn(B, n, 8, L, 4, 2, generator=g) * 3.0
    logits = torch.randn(B, n, 8, L * 4, generator=g)
    if spread_logits:                      # spread over +-40: most weights underflow
        logits = torch.rand(B, n, 8, L * 4, generator=g) * 80.0 - 40.0
    tok = 0
    for qh, qw in shapes:
        for qy in range(qh):
            for qx in range(qw):
                for l, (h, w) in enumerate(shapes):
                    bx, by = (qx + 0.5) / qw * w - 0.5, (qy + 0.5) / qh * h - 0.5
                    pix = planted_pixels(h, w)
                    for head in range(4):
                        for p in range(4):
                            off[:, tok, head, l, p, 0] = pix[p][head][0] - bx
                            off[:, tok, head, l, p, 1] = pix[p][head][1] - by
                tok += 1
    return off, logits


def msda_locations(B, shapes, Nq, seed):
    """Operator-form inputs: loc [B][Nq][8][L][4][2] in (-0.3, 1.3) with the planted pixels on
    heads 0..3 of every query ((pixel + 0.5) / (w, h), rounded to fp32), aw a softmax."""
    g = gen(seed)
    L = len(shapes)
    loc = torch.rand(B, Nq, 8, L, 4, 2, generator=g) * 1.6 - 0.3
    aw = torch.softmax(torch.randn(B, Nq, 8, L * 4, generator=g) * 2.0, -1).view(B, Nq, 8, L, 4)
    for l, (h, w) in enumerate(shapes):
        pix = planted_pixels(h, w)
        for head in range(4):
            for p in range(4):
                loc[:, :, head, l, p, 0] = (pix[p][head][0] + 0.5) / w
                loc[:, :, head, l, p, 1] = (pix[p][head][1] + 0.5) / h
    return loc, aw


# ------------------------------------------------------------------------------ fused FFN
def ffn_inputs(M, hidden, seed):
    g = gen(seed)
    u = lambda *s, a=1.0: (torch.rand(*s, generator=g) * 2.0 - 1.0) * a
    return dict(x=u(M, 256, a=2.0), W1=u(hidden, 256, a=0.1), b1=u(hidden),
                W2=u(256, hidden, a=0.05), b2=u(256), g=u(256), b=u(256), g2=u(256), b2n=u(256))


FFN_H_CHAIN = 68      # four 64-product quarters (64 roundings each, in parallel), 3 adds, + b1
