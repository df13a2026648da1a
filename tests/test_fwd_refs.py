"""CPU: the float64 statements of tests/fwd_ref.py (the references of
tests/test_fwd_kernels_gpu.py) against the functions the existing tests already trust, run in
float64 -- F.layer_norm / group_norm / normalize / gelu / interpolate, oracle.layers.msda_core,
`_attn_ref` of test_kernels_gpu.py and torch.nn.MultiheadAttention, oracle.swin.ShiftWindowMSA
with an identity projection, the patch-merging statement of test_patch_merge_ln_matches_oracle --
to 1e-12, and every condition the GPU file states about its inputs (tests/fwd_cases.py): the
planted mask rows and sampling taps are what they are named, the caps on left-out elements hold
from the reference alone, and the mutants the lab notes name would fail the named cases."""
import math

import pytest
import torch
import torch.nn.functional as F

import fwd_cases as K
import fwd_ref as R
from oracle import layers as OL
from oracle.swin import PatchMerging, ShiftWindowMSA

TOL = 1e-12
U = 2.0 ** -24
FLT_MIN = 2.0 ** -126


def _close(got, want, scale=None):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = want.abs().clamp(min=1.0) if scale is None else scale
    err = float(((got - want).abs() / scale).max())
    assert err <= TOL, err


# ------------------------------------------------------------------------------ normalisations
@pytest.mark.parametrize("rows,C", [(1, 256), (3, 256), (257, 256), (37, 4), (37, 100), (9, 3072)])
def test_layer_norm_statement_is_f_layer_norm(rows, C):
    x, kinds = K.norm_rows(rows, C, rows + C)
    g, b = K.norm_affine(C, C)
    y, mag, amp, amp2 = R.layer_norm(x, g, b, 1e-5)
    want = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5)
    _close(y, want, scale=mag.clamp_min(1e-300))
    assert bool((mag >= y.abs() * (1 - 1e-12)).all())
    for i, kd in enumerate(kinds):
        if kd == "constant":            # the statement itself gives beta (to float64 rounding)
            assert float((y[i] - b.double()).abs().max()) <= 1e-9
    # the conditioning of rstd stays a small multiple of the chain: no row kind makes the bound
    # vacuous (the offset rows carry the largest: their mean's rounding enters var squared)
    assert bool(torch.isfinite(amp).all()) and float(amp.max()) < 8.0
    assert bool(torch.isfinite(amp2).all()) and float((amp2 * 12.0 ** 2).max()) < 8.0


def test_layer_norm_mutant_one_pass_variance_fails_the_offset_rows():
    """E[x^2] - mean^2 in fp32 on a row of 1000 + 0.01 noise: the variance is lost in the
    rounding of 1e6, and the output leaves the bound the two-pass kernel is held to."""
    x, kinds = K.norm_rows(257, 256, 257 + 256)
    g, b = K.norm_affine(256, 256)
    y, mag, amp, amp2 = R.layer_norm(x, g, b, 1e-5)
    i = kinds.index("offset")
    xi = x[i]
    var1 = ((xi * xi).mean() - xi.mean() * xi.mean()).clamp_min(0.0)          # fp32, one pass
    got = (xi - xi.mean()) / torch.sqrt(var1 + 1e-5) * g + b
    c = 9.0 * (1.0 + amp[i]) + 10.0 + 81.0 * amp2[i] + 4.0
    assert bool(((got.double() - y[i]).abs() > c * U * mag[i] + FLT_MIN).any())


@pytest.mark.parametrize("HW,relu", [(1, False), (7, True), (257, False)])
def test_group_norm_statement_is_f_group_norm(HW, relu):
    x = K.groupnorm_input(2, HW, HW)
    g, b = K.norm_affine(256, 5)
    y, mag, cnt = R.group_norm_nhwc(x, g, b, 32, 1e-5, relu)
    want = F.group_norm(x.double().permute(0, 2, 1), 32, g.double(), b.double(), 1e-5)
    want = (F.relu(want) if relu else want).permute(0, 2, 1)
    _close(y, want, scale=mag.clamp_min(1e-300))
    assert float(cnt.max()) < 1.0      # the double sums cost less than one fp32 rounding
    if not relu:                       # the constant group: beta
        assert float((y[:, :, 8:16] - b.double()[8:16]).abs().max()) <= 1e-9


def test_l2_normalize_and_gelu_statements():
    x, kinds = K.l2_rows(13, 3)
    y, mag = R.l2_normalize(x, 1e-12)
    _close(y, F.normalize(x.double(), p=2, dim=-1, eps=1e-12), scale=mag.clamp_min(1e-300))
    for i, kd in enumerate(kinds):
        if kd == "zero":
            assert float(y[i].abs().max()) == 0.0
        if kd == "below_eps":
            assert float(x[i].double().norm()) < 1e-12
        if kd == "onehot":
            assert sorted(y[i].abs().tolist())[-2:] == [0.0, 1.0]
    for n in (1, 3, 1025):
        xg = K.gelu_input(n, n)
        y, mag = R.gelu(xg)
        _close(y, F.gelu(xg.double()), scale=mag.clamp_min(1e-300))


# ------------------------------------------------------------------------------ samplers
@pytest.mark.parametrize("hi,wi,ho,wo", K.BILINEAR_SIZES)
def test_bilinear_statement_is_f_interpolate_and_the_sign_cap_holds(hi, wi, ho, wo):
    x = K.bilinear_input(2, 8, hi, wi, ho, wo)[0].reshape(16, hi, wi)      # the GPU case's planes
    y, mag, spread = R.bilinear(x, ho, wo)
    want = F.interpolate(x.double()[None], (ho, wo), mode="bilinear", align_corners=False)[0]
    _close(y, want)
    if (hi, wi) == (ho, wo):
        assert torch.equal(y, x.double())
    # the stencil index of the statement reproduces the resize when blended with its weights
    idx = R.stencil_index(hi, wi, ho, wo)
    y0, y1, ly0, ly1, _ = R.taps(hi, ho)
    x0, x1, lx0, lx1, _ = R.taps(wi, wo)
    flat = x.double().reshape(16, hi * wi)
    wts = [(ly0[:, None] * lx0).reshape(-1), (ly0[:, None] * lx1).reshape(-1),
           (ly1[:, None] * lx0).reshape(-1), (ly1[:, None] * lx1).reshape(-1)]
    blend = sum(flat[:, idx[t]] * wts[t] for t in range(4)).view(16, ho, wo)
    _close(blend, want)
    # pn_bilinear_planar_gt0_u8: at most 0.1 % of the signs are decided inside the bound (torch's
    # own fp32 resize gives the allowance, exactly as the GPU test forms it)
    o32 = F.interpolate(x[None], (ho, wo), mode="bilinear", align_corners=False)[0].double()
    coord = K.bilinear_extra(hi, wi, spread)
    ratio = ((o32 - y).abs() - FLT_MIN).clamp_min(0) / (U * mag + 1e-300)
    a = max(4.0, 2.0 * float(ratio[mag > 0].max())) if bool((mag > 0).any()) else 4.0
    bound = (K.BIL_L + a) * U * mag + U * coord + FLT_MIN
    assert float((y.abs() <= bound).double().mean()) <= 1e-3


@pytest.mark.parametrize("shapes", K.MSDA_SHAPES)
def test_msda_statement_is_the_oracle_msda_core(shapes):
    B, L = 2, len(shapes)
    value = K.msda_value(B, shapes, 11 + L)
    for Nq in (1, 3, 130):
        loc, aw = K.msda_locations(B, shapes, Nq, 20 + Nq)
        out, mag, spread, ix, iy, _ = R.msda(value, shapes, loc, aw)
        want = OL.msda_core(value.double(), shapes, loc.double(), aw.double())
        _close(out, want)
        assert bool((mag >= out.abs() * (1 - 1e-12)).all())
    # the encoder form: reference points, offsets / (w, h), softmax
    off, logits = K.msda_offsets(B, shapes, 31 + L)
    loc, aw, z = R.msda_encoder_inputs(off, logits, shapes)
    n = sum(h * w for h, w in shapes)
    refs = []
    for h, w in shapes:
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64) + 0.5,
                                torch.arange(w, dtype=torch.float64) + 0.5, indexing="ij")
        refs.append(torch.stack([xx.reshape(-1) / w, yy.reshape(-1) / h], -1))
    ref = torch.cat(refs, 0)[None, :, None].repeat(B, 1, L, 1)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
    loc2 = ref[:, :, None, :, None, :] + off.double() / norm[None, None, None, :, None, :]
    aw2 = logits.double().softmax(-1).view(B, n, 8, L, 4)
    _close(loc, loc2)
    _close(aw, aw2)
    _close(R.msda(value, shapes, loc, aw)[0], OL.msda_core(value.double(), shapes, loc2, aw2))
    # the planted taps fall where they are named, to the fp32 rounding of the offset
    ix, iy = R.msda(value, shapes, loc, aw)[3:5]               # [B][N][8][L][4]
    for l, (h, w) in enumerate(shapes):
        pix = K.planted_pixels(h, w)
        for head in range(4):
            for p in range(4):
                tol = 1e-6 * (1.0 + abs(pix[p][head][0]) + abs(pix[p][head][1]))
                assert float((ix[:, :, head, l, p] - pix[p][head][0]).abs().max()) <= tol
                assert float((iy[:, :, head, l, p] - pix[p][head][1]).abs().max()) <= tol


def test_msda_zero_padding_mutant_and_far_taps():
    """A tap 1e4 pixels outside contributes exactly 0; a tap one pixel outside contributes 0 too
    (clamping it to the border instead -- the mutant -- would add the border pixel)."""
    shapes = [(3, 4)]                      # (w = 4: the planted x is exact in fp32)
    value = K.msda_value(1, shapes, 5).abs() + 1.0
    loc = torch.zeros(1, 1, 8, 1, 4, 2)
    loc[..., 0], loc[..., 1] = (-1.0 + 0.5) / 4, (1 + 0.5) / 3       # x = -1: one pixel outside
    loc[0, 0, 1, 0, :, 0] = (-1e4 + 0.5) / 4
    aw = torch.full((1, 1, 8, 1, 4), 0.25)
    out, mag, spread, _, _, _ = R.msda(value, shapes, loc, aw)
    assert float(out.abs().max()) == 0.0 and float(mag.max()) == 0.0
    assert float(spread.view(1, 1, 8, 32)[0, 0, 1].max()) == 0.0     # 1e4 outside: no neighbour
    assert float(spread.view(1, 1, 8, 32)[0, 0, 0].min()) > 0.0      # x = -1: pixel 0 is next
    clamped = value.double()[0, 4, 0]                                # row 1, column 0
    assert float(clamped.abs().min()) >= 1.0                         # the mutant's answer


# ------------------------------------------------------------------------------ attention
def _mask_of(logits, B, Q, Nk):
    return (logits < 0).view(B, Q, Nk)


@pytest.mark.parametrize("B,Q,Nk,masked", [(1, 1, 1, True), (2, 31, 33, True), (1, 33, 129, False),
                                           (2, 100, 512, True), (1, 33, 577, True)])
def test_attention_statement_is_attn_ref(B, Q, Nk, masked):
    from test_kernels_gpu import _attn_ref
    q, k, v = K.attn_inputs(B, Q, Nk, "plain", Nk)
    scale = 1 / math.sqrt(32)
    mask = _mask_of(K.mask_logits(B, Q, Nk, Nk + 1)[0], B, Q, Nk) if masked else None
    out, mag, ce, cs = R.attention(q, k, v, mask, scale)
    m2 = None
    if masked:
        m2 = mask.clone()
        m2[m2.all(-1)] = False
    _close(out, _attn_ref(q.double(), k.double(), v.double(), m2, scale))
    assert bool((mag >= out.abs() * (1 - 1e-12)).all())
    assert bool(torch.isfinite(ce).all()) and bool(torch.isfinite(cs).all())


def test_attention_statement_is_nn_multiheadattention():
    mha = torch.nn.MultiheadAttention(256, 8).double().eval()
    g = K.gen(3)
    x = torch.randn(50, 2, 256, generator=g, dtype=torch.float64)
    W, b = mha.in_proj_weight.detach(), mha.in_proj_bias.detach()
    with torch.no_grad():
        mha.out_proj.weight.copy_(torch.eye(256))
        mha.out_proj.bias.zero_()
        want = mha(x, x, x, need_weights=False)[0].transpose(0, 1)
    xb = x.transpose(0, 1)
    q, k, v = (xb @ W[i * 256:(i + 1) * 256].T + b[i * 256:(i + 1) * 256] for i in range(3))
    _close(R.attention(q, k, v, None, 1 / math.sqrt(32))[0], want)


@pytest.mark.parametrize("B,Q,Nk", [(2, 100, 33), (2, 100, 129), (2, 100, 512), (2, 100, 1100),
                                    (1, 1, 577), (2, 31, 31)])
def test_planted_mask_rows_are_what_they_are_named(B, Q, Nk):
    x, planted = K.mask_logits(B, Q, Nk, Nk + 1)
    dead = x < 0
    ch, nch = K.attn_chunking(Nk, B, Q)
    for kind, r in planted.items():
        row = dead[r]
        if kind == "all":
            assert bool(row.all())
        elif kind == "only0":
            assert not bool(row[0]) and bool(row[1:].all())
        elif kind == "onlylast":
            assert not bool(row[-1]) and bool(row[:-1].all())
        elif kind == "tile":
            assert bool(row[32:64].all()) and not bool(row[:32].any()) and not bool(row[64:].any())
        elif kind == "wave":
            tiles = list(range(1, (Nk + 31) // 32, K.attn_waves(Nk)))
            for t in range((Nk + 31) // 32):
                assert bool(row[32 * t:32 * t + 32].all()) == (t in tiles)
        elif kind == "chunk":
            assert nch >= 3 and bool(row[ch:2 * ch].all()) and not bool(row[:ch].any())
        elif kind == "block":       # one wave's 32 queries share a dead tile, alive elsewhere
            assert r == 32 and Q >= 64 and bool(dead[32:64, 64:96].all())
            assert not bool(dead[32:64].all(-1).any()) and ch == 64
    if B * Q >= 6:
        assert ("block" in planted) == (Nk > 512 and Q >= 64)
        assert {"all", "only0", "onlylast"} <= set(planted)
        if Nk > 512:
            assert "chunk" in planted
        elif Nk >= 96:
            assert "wave" in planted


def test_attention_chunking_restatement_and_the_single_chunk_case():
    assert K.attn_chunking(513, 33, 1) == (544, 1)          # one chunk: k_attn_chunk finishes
    assert K.attn_chunking(513, 2, 100)[1] > 1
    assert K.attn_chunking(16700, 1, 100) == (288, 58)
    for B, Q, Nk, _, _ in K.ATT_CASES:
        ch, nch = K.attn_chunking(Nk, B, Q)
        assert ch % 32 == 0 and ch >= 64 and (nch - 1) * ch < Nk <= nch * ch and nch <= 256


def test_attention_mutants_fail_the_named_cases():
    """From the float64 statement and the kernel's merge arithmetic: (a) without the
    running-maximum subtraction the "big" case overflows exp2; (b) a dead tile's / wave's / chunk's
    -inf maximum treated as live -- no `m_use = 0` guard, or a merge weight exp2(m - M) formed
    where both are -inf -- is exp2(-inf - -inf) = NaN, which the finiteness assertion of the bound
    catches on the rows that have such a share: "only0" / "onlylast" (every other tile dead),
    "wave" (a whole wave dead) and "chunk" (a whole chunk dead); (b') a mutant that ignores a dead
    tile's bits gives the unmasked row, far outside the "tile" row's bound; (c) dropping the last
    key of the ragged tile changes the "onlylast" row."""
    B, Q, Nk = 2, 33, 129
    q, k, v = K.attn_inputs(B, Q, Nk, "big", Nk)
    s = (q.double().view(B, Q, 8, 32).transpose(1, 2) @
         k.double().view(B, Nk, 8, 32).transpose(1, 2).transpose(-1, -2)) / math.sqrt(32)
    big = float(s.abs().amax(-1).median())
    assert 150.0 < big < 600.0                               # "about 300 in natural units"
    assert float(s.max()) * R.LOG2E > 128.0                  # (a): 2^s overflows fp32 unshifted
    # (b) the unguarded arithmetic on a share without live keys
    ninf = torch.tensor(float("-inf"))
    assert bool(torch.isnan(torch.exp2(ninf - ninf)))
    for (B_, Q_, Nk_), kind, share in (((2, 100, 129), "wave", 32 * 8), ((2, 100, 577), "chunk", 64),
                                       ((2, 100, 129), "only0", 32)):
        x, planted = K.mask_logits(B_, Q_, Nk_, Nk_ + 1)
        dead = (x < 0)[planted[kind]]
        first = 32 if kind == "wave" else 64        # the dead share starts at tile 1 / chunk 1
        step = share if kind == "wave" else Nk_     # a wave's tiles recur every NW tiles
        keys = torch.cat([torch.arange(t, min(t + 32 if kind == "wave" else t + share, Nk_))
                          for t in range(first, Nk_, step)])
        assert bool(dead[keys].all()) and not bool(dead.all())
    q, k, v = K.attn_inputs(2, 100, 129, "plain", 129)
    x, planted = K.mask_logits(2, 100, 129, 130)
    mask = _mask_of(x, 2, 100, 129)
    out, mag, ce, cs = R.attention(q, k, v, mask, 1 / math.sqrt(32))
    r = planted["tile"]
    b, qi = divmod(r, 100)
    full = R.attention(q[b:b + 1, qi:qi + 1], k[b:b + 1], v[b:b + 1], None, 1 / math.sqrt(32))[0]
    c = 200.0 + ce[b, qi]                                    # (b')
    assert bool(((full[0, 0] - out[b, qi]).abs() > c * U * mag[b, qi] + FLT_MIN).any())
    r = planted["onlylast"]
    b, qi = divmod(r, 100)
    _close(out[b, qi], v.double()[b, 128])                   # (c) the row IS the last value row
    assert float((v[b, 128] - v[b, 127]).abs().min()) > 0.0


# ------------------------------------------------------------------------------ window attention
@pytest.mark.parametrize("B,H,W,heads,ws,shift,big", K.window_cases())
def test_window_attention_statement_is_the_oracle_shift_window_msa(B, H, W, heads, ws, shift, big):
    """oracle.swin.ShiftWindowMSA in float64 with an identity output projection; the statement
    gets the module's own qkv rows.  The module pads the tokens with zeros, so a padded token's
    qkv row is the bias: the statement says so explicitly."""
    C = heads * 32
    m, x = K.window_module(B, H, W, heads, ws, shift, big, H * W + ws + shift)
    m, x = m.double(), x.double()
    with torch.no_grad():
        want = m(x, (H, W)).reshape(B * H * W, C)
        qkv = m.w_msa.qkv(x).reshape(B * H * W, 3 * C)
    table = m.w_msa.relative_position_bias_table.data.t().contiguous()
    out, mag, ce, cs = R.window_attention(qkv, m.w_msa.qkv.bias.data, table, B, H, W, C, heads, ws,
                                          shift, 32 ** -0.5)
    _close(out, want)
    assert bool((mag >= out.abs() * (1 - 1e-12)).all())
    assert bool(torch.isfinite(ce).all()) and bool(torch.isfinite(cs).all())


# ------------------------------------------------------------------------------ patch merging, FFN
@pytest.mark.parametrize("H,W", [(5, 4), (4, 5), (5, 5), (1, 1), (1, 2)])
@pytest.mark.parametrize("C", [32, 96])
def test_patch_merge_statement_is_the_oracle_patch_merging(H, W, C):
    """The statement test_patch_merge_ln_matches_oracle uses: oracle PatchMerging (nn.Unfold
    channel order c * 4 + row * 2 + col) with gamma / beta / reduction permuted to the
    neighbour-major order; and the mutant that swaps the two padded neighbours fails."""
    B = 2
    g = K.gen(H * 10 + W + C)
    pm = PatchMerging(C).double()
    pm.norm.weight.data = torch.randn(4 * C, generator=g, dtype=torch.float64) + 1.0
    pm.norm.bias.data = torch.randn(4 * C, generator=g, dtype=torch.float64)
    pm.reduction.weight.data = torch.randn(2 * C, 4 * C, generator=g, dtype=torch.float64)
    x = torch.randn(B, H * W, C, generator=g, dtype=torch.float64)
    with torch.no_grad():
        want, (h2, w2) = pm(x, (H, W))
    perm = lambda v: v.reshape(*v.shape[:-1], C, 4).transpose(-1, -2).reshape(v.shape).contiguous()
    y, mag, amp, amp2 = R.patch_merge_ln(x, perm(pm.norm.weight.data), perm(pm.norm.bias.data),
                                         B, H, W, C, 1e-5)
    assert (h2, w2) == ((H + 1) // 2, (W + 1) // 2)
    _close(y @ perm(pm.reduction.weight.data).T, want, scale=want.abs().max().clamp_min(1.0))
    rows = R.patch_merge_gather(x, B, H, W, C).view(B, h2, w2, 4, C)
    if H % 2:           # the row below the map is zero and enters the statistics as zeros
        assert float(rows[:, -1, :, 2:].abs().max()) == 0.0
    if W % 2:
        assert float(rows[:, :, -1, 1::2].abs().max()) == 0.0
    if H % 2 != W % 2:  # swapping neighbours 1 (right) and 2 (below) moves the zeros
        swapped = rows[:, :, :, [0, 2, 1, 3]].reshape(B, h2 * w2, 4 * C)
        y2 = R.layer_norm(swapped, perm(pm.norm.weight.data), perm(pm.norm.bias.data), 1e-5)[0]
        assert float((y2 - y).abs().max()) > 1e-3


@pytest.mark.parametrize("M,hidden", [(1, 64), (33, 128), (100, 2048)])
def test_ffn_statement_and_the_relu_cap(M, hidden):
    p = K.ffn_inputs(M, hidden, M + hidden)
    u, umag, h, hmag = R.ffn_pre(p["x"], p["W1"], p["b1"], p["W2"], p["b2"])
    d = lambda t: t.double()
    want = d(p["x"]) + F.linear(F.relu(F.linear(d(p["x"]), d(p["W1"]), d(p["b1"]))), d(p["W2"]),
                                d(p["b2"]))
    _close(u, want)
    y, mag, amp, amp2 = R.layer_norm(u, p["g"], p["b"], 1e-5, xmag=umag)
    _close(y, F.layer_norm(want, (256,), d(p["g"]), d(p["b"]), 1e-5))
    assert bool((umag >= u.abs() * (1 - 1e-12)).all())
    # ReLU inputs within their own bound of zero: at most 0.1 % (they are compared all the same:
    # ReLU is 1-Lipschitz and umag is built on hmag)
    near = h.abs() <= (K.FFN_H_CHAIN + 4.0) * U * hmag + FLT_MIN
    assert float(near.double().mean()) <= 1e-3
    chain = K.FFN_H_CHAIN + 64 + hidden // 64 + 2
    assert float(amp.max()) < 8.0 and float((amp2 * chain ** 2).max()) < 8.0
