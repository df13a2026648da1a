"""GPU: the forward kernels every inference step and every taped forward run through -- the
softmax attentions (pn_attention_f32 with pn_mask_pack, pn_window_attention_f32), the
normalisations (pn_layernorm_f32, pn_layernorm_rows_f32 / _s3, pn_patch_merge_ln_f32,
pn_groupnorm_nhwc_f32, pn_groupnorm_upadd_nhwc_f32, pn_l2normalize_f32), the samplers (pn_msda_f32,
pn_msda_loc_f32, pn_bilinear_nhwc / planar / planar_gt0 / stencil_rows), the fused FFN
(pn_ffn_ln_f32 / pn_ffn_ln2_f32) and pn_gelu_f32 -- one at a time against the float64 statements
of tests/fwd_ref.py (pinned to torch / the oracle without a GPU by tests/test_fwd_refs.py), on the
inputs of tests/fwd_cases.py: the smallest shapes that reach every branch, and the values at which
this arithmetic goes wrong.

Bounds.  |got - ref| <= (L + a + cond) 2^-24 mag + 2^-24 extra + FLT_MIN on every output element.
  mag    the float64 computation on absolute values;
  L      the longest chain of fp32 roundings the element passes through, counted from the kernel's
         source and written as a formula of the shape beside each test (labnotes/r19.md has the
         table, written before the first run);
  cond   where an exponential or a reciprocal square root sits between input and output: the
         roundings it multiplies, per element, from the inputs alone (fwd_ref.py states each); the
         softmax's score term cnt_score enters the large-score cases only;
  extra  where a sampling coordinate is rounded: k 2^-24 (1 + |coordinate| + max(h, w)) of a pixel
         times the largest difference between the taps, per element, from the inputs alone;
  a      max(4, 2 x the ratio torch's own fp32 evaluation of the same operation reaches on the same
         inputs against the same reference and mag, net of cond and extra).
Nothing in the bound comes from the kernel under test.  Every case prints the kernel's and the
fp32 oracle's plain ratio |err| / (2^-24 (mag + extra)), the oracle's net of cond, and
c = L + a + cond; the worst of each per kernel is printed when the module ends.  Data movement,
untouched outputs, NaN fences and refused calls are compared bitwise; every
kernel is launched twice and must give equal bits."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fwd_cases as K
import fwd_ref as R
from test_grad_kernels_gpu import FLT_MIN, U, _gen, _randn, _within, _within_rows  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
NAN_BITS = 0x7fc00000
WORST = {}          # kernel -> (kernel ratio, fp32-oracle ratio, c, case); plain ratios


@pytest.fixture(scope="module")
def hip(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip as h
    h.lib()
    yield h
    print("\n%-26s %12s %14s %10s  case" % ("kernel", "worst ratio", "fp32 oracle", "c"))
    for k, (r, o, c, case) in sorted(WORST.items()):
        print("%-26s %12.3f %14.3f %10.4g  %s" % (k, r, o, c, case))


def _d(t):
    return t.to(DEV)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _is_fence(t):
    """Every element still has the NaN fill, bit for bit."""
    return bool((_bits(t) == NAN_BITS).all())


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ratio(got, ref, mag, allow):
    """Largest (|got - ref| - FLT_MIN - allow) / (2^-24 mag), `allow` the part of the bound that
    conditioning (cond, extra) grants; inf where that is positive at mag = 0."""
    err = (got.detach().to(DEV).double() - ref).abs() - FLT_MIN - allow
    err = err.clamp_min(0.0)
    ratio = torch.where(err > 0, err / (U * mag), torch.zeros_like(err))
    return float(ratio.max()) if ratio.numel() else 0.0


def _note(kernel, case, worst, oracle, c):
    if kernel not in WORST or worst > WORST[kernel][0]:
        WORST[kernel] = (worst, oracle, c, case)


def _full(t, shape):
    t = torch.as_tensor(t, dtype=torch.float64, device=DEV)
    return t.expand(shape) if t.dim() == 0 else t.to(DEV).double().reshape(shape)


def _bounded(kernel, case, got, ref, mag, L, o32, cond=None, extra=None):
    """Asserts |got - ref| <= (L + a + cond) 2^-24 mag + 2^-24 extra + FLT_MIN element-wise with
    a = max(4, 2 x the fp32 oracle's ratio); L and cond may be tensors (a count per element).
    Returns (the kernel's worst ratio, a)."""
    shape = got.shape
    ref, mag = _full(ref, shape), _full(mag, shape)
    cond = _full(cond, shape) if cond is not None else torch.zeros_like(mag)
    extra = _full(extra, shape) if extra is not None else torch.zeros_like(mag)
    count = _full(L, shape) + cond
    allow = U * (cond * mag + extra)            # the conditioning, from the inputs alone
    oracle = _ratio(o32.reshape(shape), ref, mag, allow)
    a = max(4.0, 2.0 * oracle) if math.isfinite(oracle) else 4.0
    cmax = float(count.max()) + a
    # the plain ratios |err| / (2^-24 (mag + extra)), for the table
    zero = torch.zeros_like(mag)
    raw, raw_o = _ratio(got, ref, mag + extra, zero), _ratio(o32.reshape(shape), ref, mag + extra, zero)
    print("%-66s |err| / (2^-24 mag): kernel %9.3f  fp32 oracle %9.3f (net of cond %7.3f)  "
          "L + cond <= %-9.5g c <= %.5g" % (kernel + " " + case, raw, raw_o, oracle,
                                            float(count.max()), cmax))
    worst = _within(kernel + " " + case, got, ref, mag * ((count + a) / cmax) + extra / cmax, cmax)
    _note(kernel, case, raw, raw_o, cmax)
    return worst, a


def _strided(x, extra):
    """x [rows][cols] as a column slice of a buffer `extra` columns wider, NaN beyond it."""
    wide = _nan(x.shape[0], x.shape[1] + extra)
    wide[:, :x.shape[1]] = x
    return wide, wide[:, :x.shape[1]]


# ============================================================ pn_attention_f32 + pn_mask_pack
def _attn_chain(B, Q, Nk):
    """L of pn_attention_f32 beyond the score (which cond carries).  Per numerator p_j v_jd and
    the denominator, with T tiles per wave / chunk and W partials merged:
      exp2 evaluations (v_exp_f32, 1 ulp = 2 roundings): p, T - 1 running-maximum rescales, the
        merge weight                                                     2 (T + 1)
      rescale products on the numerator                                  T
      numerator sum: 32 keys per tile through the MFMA                   32 T
      denominator: 16 in-lane adds, (x alpha, + psum) per tile, xor-32   16 + 2 T + 1
      merge: (x weight, add) per partial on numerator and denominator    merge(W)
      1 / den and the final product                                      2
    k_attn_small: T = ceil(tiles / NW), W = NW, merge = 4 W.
    k_attn_chunk + k_attn_combine: T = chunk / 32; numerator: ceil(W / 16) (x, +) in each of four
      accumulators, 2 adds, 3 phase adds; denominator: ceil(W / 128) (x, +), 5 shuffle adds, 3
      phase adds; the quotient: merge = 2 ceil(W / 16) + 2 ceil(W / 128) + 14.  One chunk: 0."""
    if Nk <= K.ATT_SMALL_MAX:
        NW = K.attn_waves(Nk)
        T, merge = -(-((Nk + 31) // 32) // NW), 4 * NW
    else:
        ch, W = K.attn_chunking(Nk, B, Q)
        T = ch // 32
        merge = 0 if W == 1 else 2 * -(-W // 16) + 2 * -(-W // 128) + 14
    return 2 * (T + 1) + T + 32 * T + 16 + 2 * T + 1 + merge + 2


def _attn_o32(q, k, v, mask, scale):
    from test_kernels_gpu import _attn_ref
    m2 = None
    if mask is not None:
        m2 = mask.clone()
        m2[m2.all(-1)] = False
    return _attn_ref(q, k, v, m2, scale)


def _pack(hip, logits, B, Q, Nk):
    """pn_mask_pack of logits [B*Q][Nk] -> (bits, rowall), checked bit for bit against numpy
    inside fenced buffers."""
    R_, nw = B * Q, (Nk + 31) // 32
    runs = []
    for fill in (0x5a5a5a5a, 0x25a5a5a5):            # two launches over different garbage
        bits = torch.full((R_ * nw + 8,), fill, device=DEV, dtype=torch.int32)
        rowall = torch.full((R_ + 8,), 7, device=DEV, dtype=torch.int32)
        hip.mask_pack(logits, bits, rowall, R_, Nk)
        torch.cuda.synchronize()
        assert bool((bits[R_ * nw:] == fill).all()) and bool((rowall[R_:] == 7).all())
        runs.append((bits, rowall))
    assert torch.equal(runs[0][0][:R_ * nw], bits[:R_ * nw]) and \
        torch.equal(runs[0][1][:R_], rowall[:R_]), "pn_mask_pack is not bitwise reproducible"
    dead = (logits < 0).cpu()
    words = bits[:R_ * nw].cpu().view(R_, nw).numpy().view(np.uint32)
    unpacked = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")
    assert np.array_equal(unpacked[:, :Nk].astype(bool), dead.numpy())
    assert torch.equal(rowall[:R_].cpu(), dead.all(-1).to(torch.int32))
    return bits, rowall


@pytest.mark.parametrize("B,Q,Nk,masked,kind", K.ATT_CASES)
def test_fwd_attention(hip, B, Q, Nk, masked, kind):
    q, k, v = (_d(t) for t in K.attn_inputs(B, Q, Nk, kind, Nk))
    scale = 1 / math.sqrt(32)
    mask = bits = rowall = None
    if masked:
        logits = _d(K.mask_logits(B, Q, Nk, Nk + 1)[0])
        bits, rowall = _pack(hip, logits, B, Q, Nk)
        mask = (logits < 0).view(B, Q, Nk)
    stated = hip.attn_scratch_floats(B, Q, Nk)
    ch, nch = K.attn_chunking(Nk, B, Q)
    # what the launch may touch: per (image, head, chunk, query) 32 numerators + (m, l)
    assert stated == (64 if Nk <= K.ATT_SMALL_MAX else B * 8 * nch * Q * 34)
    ldo = 320
    outs = []
    for _ in range(2):
        scr, out = _nan(stated + 64), _nan(B * Q, ldo)
        hip.attention(q.view(-1, 256), 256, k.view(-1, 256), 256, v.view(-1, 256), 256, bits, rowall,
                      out, ldo, scr, B, Q, Nk, scale)
        torch.cuda.synchronize()
        assert _is_fence(scr[stated:]), "wrote past pn_attn_scratch_floats"
        assert _is_fence(out[:, 256:]), "wrote the unused columns of a wide out"
        outs.append(out[:, :256])
    assert _same_bits(outs[0], outs[1]), "pn_attention_f32 is not bitwise reproducible"
    ref, mag, ce, cs = R.attention(q, k, v, mask, scale)
    kernel = "k_attn_small<%d>" % K.attn_waves(Nk) if Nk <= K.ATT_SMALL_MAX else \
        ("k_attn_chunk" if nch == 1 else "k_attn_chunk+combine")
    _bounded(kernel, "B %d Q %d Nk %d masked %d %s" % (B, Q, Nk, masked, kind),
             outs[0].reshape(B, Q, 256), ref, mag, _attn_chain(B, Q, Nk),
             _attn_o32(q, k, v, mask, scale), cond=ce + cs if kind == "big" else ce)


def test_fwd_attention_strided_packed_qk(hip):
    """Self-attention as the decoder issues it: q and k are the two halves of one [Q | K] buffer
    with ld 512, v has ld 256, out a column window of a wider buffer (ldo 384 > 256)."""
    B, Q = 2, 100
    QK, V = (_d(t) for t in K.attn_packed_inputs(B, Q, 5))
    scale = 1 / math.sqrt(32)
    outs = []
    for _ in range(2):
        out = _nan(B * Q, 384)
        scr = _nan(hip.attn_scratch_floats(B, Q, Q) + 64)
        hip.attention(QK, 512, QK[:, 256:], 512, V, 256, None, None, out, 384, scr, B, Q, Q, scale)
        torch.cuda.synchronize()
        assert _is_fence(out[:, 256:]) and _is_fence(scr[hip.attn_scratch_floats(B, Q, Q):])
        outs.append(out[:, :256])
    assert _same_bits(outs[0], outs[1])
    q, k, v = (t.reshape(B, Q, 256) for t in (QK[:, :256], QK[:, 256:], V))
    ref, mag, ce, cs = R.attention(q, k, v, None, scale)
    _bounded("k_attn_small<4>", "packed [Q|K] ld 512, ldo 384", outs[0].reshape(B, Q, 256), ref,
             mag, _attn_chain(B, Q, Q), _attn_o32(q, k, v, None, scale), cond=ce)


# ============================================================ pn_window_attention_f32
@pytest.mark.parametrize("B,H,W,heads,ws,shift,big", K.window_cases())
def test_fwd_window_attention(hip, B, H, W, heads, ws, shift, big):
    """L: as _attn_chain with every key tile in one wave (T = ceil(ws^2 / 32), nothing merged),
    + 2 for the bias and region-mask additions.  The score term cnt_score (the bias table's
    x log2(e) rounding and |bias| are in its E) enters the case with bias entries of +-30 only."""
    C, n = heads * 32, B * H * W
    m, x = K.window_module(B, H, W, heads, ws, shift, big, H * W + ws + shift)
    with torch.no_grad():
        o32 = m(x, (H, W)).reshape(n, C)
        qkv = m.w_msa.qkv(x).reshape(n, 3 * C)
    bias = _d(m.w_msa.qkv.bias.data)
    table = _d(m.w_msa.relative_position_bias_table.data.t().contiguous())
    wide, view = _strided(_d(qkv), 8)                        # ldqkv = 3C + 8
    outs = []
    for _ in range(2):
        out = _nan(n, C + 4)                                 # ldo = C + 4
        hip.window_attention(view, bias, table, out[:, :C], B, H, W, C, heads, ws, shift)
        torch.cuda.synchronize()
        assert _is_fence(out[:, C:])
        outs.append(out[:, :C])
    assert _same_bits(outs[0], outs[1])
    ref, mag, ce, cs = R.window_attention(_d(qkv), bias, table, B, H, W, C, heads, ws, shift,
                                          32 ** -0.5)
    T = (ws * ws + 31) // 32
    L = 2 * (T + 1) + T + 32 * T + 16 + 2 * T + 1 + 2 + 2
    _bounded("k_window_attn", "B %d %dx%d heads %d ws %d shift %d bias30 %d" % (
        B, H, W, heads, ws, shift, big), outs[0], ref, mag, L, _d(o32), cond=ce + cs if big else ce)


# ============================================================ LayerNorm
def _ln_count(chain, fixed, amp, amp2):
    """chain roundings on d = x - mean (relative to |x| + mean |x|) reach the output directly and
    through rstd: chain (1 + amp) + chain^2 amp2 (fwd_ref.layer_norm); `fixed`: rstd's own
    roundings and the three of (d rstd) gamma + beta."""
    return chain * (1.0 + amp) + chain * chain * amp2 + fixed


LN256_CHAIN = 9     # mean: 2 in-lane adds, 6 wave steps (x 1/256 is exact); x - mean
LN256_FIXED = 10    # var: square, 2 + 6 adds, + eps = 10 -> 5 on rstd, sqrt, 1 / ; x rstd, x g, + b


@pytest.mark.parametrize("rows", [1, 3, 255, 257])
def test_fwd_layernorm256(hip, rows):
    x, kinds = K.norm_rows(rows, 256, rows + 256)
    g, b = K.norm_affine(256, 256)
    x, g, b = _d(x), _d(g), _d(b)
    outs = []
    for _ in range(2):
        out = _nan(rows + 1, 256)
        hip.layernorm(x, g, b, out[:rows])
        torch.cuda.synchronize()
        assert _is_fence(out[rows:])
        outs.append(out[:rows])
    assert _same_bits(outs[0], outs[1])
    for i, kd in enumerate(kinds):       # equal addends sum exactly in the power-of-two tree
        if kd == "constant":
            assert torch.equal(outs[0][i], b), "a constant row must give beta exactly"
    ref, mag, amp, amp2 = R.layer_norm(x, g, b, 1e-5)
    _bounded("k_layernorm256", "rows %d" % rows, outs[0], ref, mag,
             _ln_count(LN256_CHAIN, LN256_FIXED, amp, amp2), F.layer_norm(x, (256,), g, b, 1e-5))


def _ln_rows_counts(C):
    """k_ln_rows with nv = ceil(C / 256) float4s per lane.  mean: 2 adds per float4 and nv
    accumulations in the lane, 6 wave steps, / C; x - mean: chain nv + 10.  var: square, the
    same sum, / C, + eps = nv + 11 -> half of it on rstd, sqrt, 1 / ; then x rstd, x g, + b."""
    nv = (C + 255) // 256
    return nv + 10, math.ceil(0.5 * (nv + 11)) + 2 + 3


@pytest.mark.parametrize("C", [4, 96, 100, 1536, 3072])
def test_fwd_layernorm_rows(hip, C):
    """Rows of every kind in a column window (ldx = C + 8, ldy = C + 4).  The constant rows hold
    -3: k_ln_rows adds 3, 6, 12 .. equal addends in a lane and 24 lanes' worth at C = 96, so only
    a value with spare mantissa bits sums exactly there (the 256-wide kernel's tree is exact for
    any value)."""
    rows = 37
    x, kinds = K.norm_rows(rows, C, rows + C, const=-3.0)
    g, b = K.norm_affine(C, C)
    g, b = _d(g), _d(b)
    _, xv = _strided(_d(x), 8)
    outs = []
    for _ in range(2):
        out = _nan(rows, C + 4)
        hip.layernorm_rows(xv, g, b, out[:, :C])
        torch.cuda.synchronize()
        assert _is_fence(out[:, C:])
        outs.append(out[:, :C])
    assert _same_bits(outs[0], outs[1])
    for i, kd in enumerate(kinds):
        if kd == "constant":
            assert torch.equal(outs[0][i], b)
    ref, mag, amp, amp2 = R.layer_norm(xv, g, b, 1e-5)
    chain, fixed = _ln_rows_counts(C)
    _bounded("k_ln_rows", "C %d rows %d" % (C, rows), outs[0], ref, mag,
             _ln_count(chain, fixed, amp, amp2), F.layer_norm(xv, (C,), g, b, 1e-5))


@pytest.mark.parametrize("rows,C", [(37, 96), (64, 1536), (33, 256)])
def test_fwd_layernorm_rows_s3_is_the_split_of_the_fp32_rows(hip, rows, C):
    x, _ = K.norm_rows(rows, C, rows + C, const=-3.0)
    g, b = K.norm_affine(C, C)
    g, b = _d(g), _d(b)
    _, xv = _strided(_d(x), 16)
    y = _nan(rows, C)
    hip.layernorm_rows(xv, g, b, y)
    want = torch.zeros(hip.s3_floats(rows, C), device=DEV)
    hip.s3_split(y, want)
    got, again = torch.zeros_like(want), torch.zeros_like(want)
    hip.layernorm_rows_s3(xv, g, b, got)
    hip.layernorm_rows_s3(xv, g, b, again)
    back = _nan(rows, C)
    hip.s3_join(got, back)
    torch.cuda.synchronize()
    assert _same_bits(got, want) and _same_bits(again, want) and _same_bits(back, y)


@pytest.mark.parametrize("H,W", [(5, 4), (4, 5), (5, 5), (1, 1), (1, 2)])
@pytest.mark.parametrize("C", [32, 96])
def test_fwd_patch_merge_ln(hip, H, W, C):
    """k_ln_rows<merge>: the counts of k_ln_rows at width 4C; the zero-padded neighbours of an
    odd map enter the statistics as zeros (fwd_ref.patch_merge_gather)."""
    B = 2
    x = _d(K.patch_merge_input(B, H, W, C, H * 10 + W + C))
    g, b = (_d(t) for t in K.norm_affine(4 * C, C))
    n2 = B * ((H + 1) // 2) * ((W + 1) // 2)
    outs = []
    for _ in range(2):
        out = _nan(n2 + 1, 4 * C)
        hip.patch_merge_ln(x, g, b, out[:n2], B, H, W, C)
        torch.cuda.synchronize()
        assert _is_fence(out[n2:])
        outs.append(out[:n2])
    assert _same_bits(outs[0], outs[1])
    ref, mag, amp, amp2 = R.patch_merge_ln(x, g, b, B, H, W, C, 1e-5)
    rows32 = R.patch_merge_gather(x, B, H, W, C).float()
    chain, fixed = _ln_rows_counts(4 * C)
    _bounded("k_ln_rows<merge>", "%dx%d C %d" % (H, W, C), outs[0], ref.reshape(n2, 4 * C),
             mag.reshape(n2, 4 * C), _ln_count(chain, fixed, amp, amp2).reshape(n2, 4 * C),
             F.layer_norm(rows32, (4 * C,), g, b, 1e-5))


# ============================================================ GroupNorm
GN_L = 6   # the partial sums are double: (float) mean, x - mean, (float) rstd, x rstd, x g, + b


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("HW", [1, 7, 256, 257])       # pn_groupnorm_nblk steps from 256 to 257
def test_fwd_groupnorm_nhwc(hip, HW, relu):
    B, G = 2, 32
    assert hip.groupnorm_nblk(256) == 1 and hip.groupnorm_nblk(257) == 2
    x = _d(K.groupnorm_input(B, HW, HW))
    g, b = (_d(t) for t in K.norm_affine(256, 5))
    xin = _nan(B, HW + 3, 256)                             # batch strides on both sides
    xin[:, :HW] = x
    nblk = hip.groupnorm_nblk(HW)
    outs = []
    for _ in range(2):
        out = _nan(B, HW + 5, 256)
        part = torch.full((B * nblk * 64 + 8,), NAN, device=DEV, dtype=torch.float64)
        hip.groupnorm_nhwc(xin, g, b, out, part, B, HW, G, relu, (HW + 3) * 256, (HW + 5) * 256)
        torch.cuda.synchronize()
        assert _is_fence(out[:, HW:]) and bool(torch.isnan(part[B * nblk * 64:]).all())
        outs.append(out[:, :HW])
    assert _same_bits(outs[0], outs[1])
    want_const = b[8:16].clamp_min(0.0) if relu else b[8:16]
    assert torch.equal(outs[0][:, :, 8:16], want_const.expand(B, HW, 8)), \
        "a constant group must give beta exactly"
    ref, mag, cnt = R.group_norm_nhwc(x, g, b, G, 1e-5, relu)
    o32 = F.group_norm(x.permute(0, 2, 1), G, g, b, 1e-5)
    o32 = (F.relu(o32) if relu else o32).permute(0, 2, 1)
    _bounded("k_gn_partial+k_gn_apply", "HW %d relu %d" % (HW, relu), outs[0], ref, mag, GN_L, o32,
             cond=cnt)


BIL_L, BIL_COORD, _bil_extra = K.BIL_L, K.BIL_COORD, K.bilinear_extra


def test_fwd_groupnorm_upadd(hip):
    """y = GroupNorm(x) + bilinear-up(coarse) on a small odd map, against float64 GroupNorm plus
    float64 bilinear: the two terms' counts on their own mags, + 1 for the add."""
    B, H, W, hc, wc, G = 2, 5, 7, 3, 4, 32
    x = _d(K.groupnorm_input(B, H * W, 41))
    g, b = (_d(t) for t in K.norm_affine(256, 6))
    coarse = _d(K.upadd_coarse(B, hc, wc, 42))
    nblk = hip.groupnorm_nblk(H * W)
    outs = []
    for _ in range(2):
        part = torch.full((B * nblk * 64 + 8,), NAN, device=DEV, dtype=torch.float64)
        out = _nan(B, H * W + 2, 256)
        hip.groupnorm_upadd_nhwc(x, g, b, out, part, coarse, B, H, W, hc, wc, G, H * W * 256,
                                 (H * W + 2) * 256, hc * wc * 256)
        torch.cuda.synchronize()
        assert _is_fence(out[:, H * W:]) and bool(torch.isnan(part[B * nblk * 64:]).all())
        outs.append(out[:, :H * W])
    assert _same_bits(outs[0], outs[1])
    gn, gmag, cnt = R.group_norm_nhwc(x, g, b, G, 1e-5, False)
    cmap = coarse.view(B, hc, wc, 256).permute(0, 3, 1, 2)
    up, umag, spread = R.bilinear(cmap, H, W)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(B, H * W, 256)
    up, umag, spread = nhwc(up), nhwc(umag), nhwc(spread)
    mag = gmag + umag
    count = ((GN_L + cnt) * gmag + BIL_L * umag) / mag.clamp_min(1e-300) + 1.0
    o32 = F.group_norm(x.permute(0, 2, 1), G, g, b, 1e-5).permute(0, 2, 1) + \
        nhwc(F.interpolate(cmap, (H, W), mode="bilinear", align_corners=False))
    _bounded("k_gn_apply_up", "5x7 <- 3x4", outs[0], gn + up, mag, count, o32,
             extra=_bil_extra(hc, wc, spread))


# ============================================================ l2 normalise, GELU
def test_fwd_l2normalize(hip):
    """L = 7: squares and the in-lane / wave sum 9 -> 5 on the norm, sqrt, the quotient.  Rows
    of zeros give exactly 0; one-hot rows exactly +-1 (sqrt(fl(v^2)) = |v| with a correctly
    rounded square root); rows below eps are x / eps."""
    rows = 13
    x, kinds = K.l2_rows(rows, 3)
    x = _d(x)
    outs = []
    for _ in range(2):
        out = _nan(rows + 1, 256)
        hip.l2normalize(x, out[:rows])
        torch.cuda.synchronize()
        assert _is_fence(out[rows:])
        outs.append(out[:rows])
    assert _same_bits(outs[0], outs[1])
    for i, kd in enumerate(kinds):
        if kd == "zero":
            assert bool((outs[0][i] == 0).all())
        if kd == "onehot":
            assert torch.equal(outs[0][i], torch.sign(x[i]))
    ref, mag = R.l2_normalize(x, 1e-12)
    _bounded("k_l2norm256", "rows %d" % rows, outs[0], ref, mag, 7,
             F.normalize(x, p=2, dim=-1, eps=1e-12))


@pytest.mark.parametrize("n", [1, 3, 1025])
def test_fwd_gelu(hip, n):
    """L = 3: x / sqrt 2, 1 + erf, the product (0.5 x is exact); erff itself is the allowance."""
    x = _d(K.gelu_input(n, n))
    outs = []
    for _ in range(2):
        out = _nan(n + 1)
        hip.gelu(x, out[:n])
        torch.cuda.synchronize()
        assert _is_fence(out[n:])
        outs.append(out[:n])
    assert _same_bits(outs[0], outs[1])
    ref, mag = R.gelu(x)
    _bounded("k_gelu", "n %d" % n, outs[0], ref, mag, 3, F.gelu(x))


# ============================================================ bilinear resize
@pytest.mark.parametrize("hi,wi,ho,wo", K.BILINEAR_SIZES)
def test_fwd_bilinear(hip, hi, wi, ho, wo):
    """pn_bilinear_nhwc_f32 (plain and accumulating, batch strides), pn_bilinear_planar_f32,
    pn_bilinear_planar_gt0_u8 and pn_bilinear_stencil_rows_f32 on one map.  Equal sizes are the
    identity, exactly."""
    B, C = 2, 8
    x, base = (_d(t) for t in K.bilinear_input(B, C, hi, wi, ho, wo))   # planes [B * C][hi][wi]
    ref, mag, spread = R.bilinear(x, ho, wo)
    extra = _bil_extra(hi, wi, spread)
    o32 = F.interpolate(x, (ho, wo), mode="bilinear", align_corners=False)
    case = "%dx%d -> %dx%d" % (hi, wi, ho, wo)
    # ---- planar
    outs = []
    for _ in range(2):
        out = _nan(B * C * ho * wo + 4)
        hip.bilinear_planar(x, out, B * C, hi, wi, ho, wo)
        torch.cuda.synchronize()
        assert _is_fence(out[B * C * ho * wo:])
        outs.append(out[:B * C * ho * wo].view(B, C, ho, wo))
    assert _same_bits(outs[0], outs[1])
    if (hi, wi) == (ho, wo):
        assert torch.equal(outs[0], x)
    _, a = _bounded("k_bilinear_planar", case, outs[0], ref, mag, BIL_L, o32, extra=extra)
    # ---- the sign map: every element whose reference is outside its own bound must agree
    o8s = []
    for fill in (9, 7):
        o8 = torch.full((B * C * ho * wo + 4,), fill, device=DEV, dtype=torch.uint8)
        hip.bilinear_planar_gt0(x, o8, B * C, hi, wi, ho, wo)
        torch.cuda.synchronize()
        assert bool((o8[B * C * ho * wo:] == fill).all())
        o8s.append(o8[:B * C * ho * wo])
    assert torch.equal(o8s[0], o8s[1])
    inside = ref.abs() <= (BIL_L + a) * U * mag + U * extra + FLT_MIN
    assert float(inside.double().mean()) <= 1e-3
    got8 = o8[:B * C * ho * wo].view(B, C, ho, wo)
    assert bool((got8 <= 1).all()) and bool(((got8 == 1) == (ref > 0))[~inside].all())
    assert torch.equal(got8 == 1, outs[0] > 0)                     # the same blend, thresholded
    # ---- channel-last, batch strides, plain and accumulating (one more rounding)
    xin = _nan(B, hi * wi + 3, C)
    xin[:, :hi * wi] = x.permute(0, 2, 3, 1).reshape(B, hi * wi, C)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(B, ho * wo, C)
    for acc in (False, True):
        outs = []
        for _ in range(2):
            out = _nan(B, ho * wo + 5, C)
            if acc:
                out[:, :ho * wo] = base
            hip.bilinear_nhwc(xin, out, B, hi, wi, ho, wo, C, acc, (hi * wi + 3) * C,
                              (ho * wo + 5) * C)
            torch.cuda.synchronize()
            assert _is_fence(out[:, ho * wo:])
            outs.append(out[:, :ho * wo])
        assert _same_bits(outs[0], outs[1])
        r, m_, o = nhwc(ref), nhwc(mag), nhwc(o32)
        if acc:
            r, m_, o = r + base.double(), m_ + base.double().abs(), o + base
        _bounded("k_bilinear_nhwc", case + (" accumulate" if acc else ""), outs[0], r, m_,
                 BIL_L + int(acc), o, extra=nhwc(extra))
    # ---- stencil rows: a gather by the statement's tap indices, bit for bit.  Where a source
    # coordinate lies within its fp32 rounding of an integer the floor may fall either side:
    # there the row must equal the gather by one of the two neighbouring index choices (the
    # blend below is indifferent: the tap that changes has weight ~0).
    both = []
    for _ in range(2):
        rows = _nan(B, 4 * ho * wo + 1, C)
        hip.bilinear_stencil_rows(xin, rows, B, hi, wi, ho, wo, C, (hi * wi + 3) * C,
                                  (4 * ho * wo + 1) * C)
        torch.cuda.synchronize()
        assert _is_fence(rows[:, 4 * ho * wo:])
        both.append(rows[:, :4 * ho * wo])
    assert _same_bits(both[0], both[1])
    rows = both[0]
    tol = BIL_COORD * U * (1.0 + max(hi, wi))
    ok = torch.zeros(B, 4 * ho * wo, dtype=torch.bool, device=DEV)
    for nudge in (0.0, -tol, tol):
        idx = _d(R.stencil_index(hi, wi, ho, wo, nudge).reshape(-1))
        ok |= (_bits(rows) == _bits(xin[:, idx])).all(-1)
        if nudge == 0.0:
            assert float(ok.double().mean()) >= 0.9
    assert bool(ok.all()), "stencil rows are not the statement's taps"
    y0, y1, ly0, ly1, _ = R.taps(hi, ho, DEV)
    x0, x1, lx0, lx1, _ = R.taps(wi, wo, DEV)
    wts = torch.stack([(ly0[:, None] * lx0).reshape(-1), (ly0[:, None] * lx1).reshape(-1),
                       (ly1[:, None] * lx0).reshape(-1), (ly1[:, None] * lx1).reshape(-1)])
    blend = (rows.double().view(B, 4, ho * wo, C) * wts[None, :, :, None]).sum(1)
    _within("stencil rows blended " + case, blend, nhwc(ref),
            nhwc(mag) + nhwc(extra) / BIL_COORD, BIL_COORD * 1.0)


# ============================================================ deformable sampling
MSDA_COORD = 7      # ref = (q + 0.5) / qw, off / w, +, 2 loc - 1, + 1, x w, - 1 (x 0.5 is exact)
MSDA_LOC_COORD = 4  # 2 loc - 1, + 1, x w, - 1


def _msda_chain(L):
    """Weights (1 - t), product: 2; four tap products and three adds, the first product and add
    fused by the chain: 4; x attention weight 1; the sum over L levels L; two point shuffles 2;
    the softmax: x - max (carried by cond), L + 1 adds of the denominator, the quotient: L + 3."""
    return 2 + 4 + 1 + L + 2 + L + 3


def _offaw(off, logits):
    B, n = off.shape[:2]
    return torch.cat([off.reshape(B, n, -1), logits.reshape(B, n, -1)], -1).contiguous()


def _msda_o32(value, off, logits, shapes):
    """torch's fp32 evaluation: the oracle's msda_core on locations and weights formed in fp32 the
    way test_kernels_gpu._msda_ref forms them."""
    from oracle import layers as OL
    B, n = value.shape[:2]
    refs = []
    for h, w in shapes:
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=DEV) + 0.5,
                                torch.arange(w, dtype=torch.float32, device=DEV) + 0.5, indexing="ij")
        refs.append(torch.stack([xx.reshape(-1) / w, yy.reshape(-1) / h], -1))
    ref = torch.cat(refs, 0)[None, :, None].repeat(B, 1, len(shapes), 1)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32, device=DEV)
    loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    aw = logits.softmax(-1).view(B, n, 8, len(shapes), 4)
    return OL.msda_core(value, shapes, loc, aw)


@pytest.mark.parametrize("spread_logits", [False, True])
@pytest.mark.parametrize("shapes", K.MSDA_SHAPES)
def test_fwd_msda(hip, shapes, spread_logits):
    """pn_msda_f32 on 1 / 2 / 4 levels with 1 x 1, 1 x 5, 5 x 1 maps, B = 2, odd N, taps planted on
    pixel centres, on -0.5, on the far edges, one pixel and 1e4 pixels outside (heads 0..3) and
    logits spread over +-40."""
    B, L = 2, len(shapes)
    n = sum(h * w for h, w in shapes)
    assert n % 2 == 1
    value = _d(K.msda_value(B, shapes, 11 + L))
    off, logits = (_d(t) for t in K.msda_offsets(B, shapes, 31 + L, spread_logits))
    offaw = _offaw(off, logits)
    outs = []
    for _ in range(2):
        out = _nan(B * n + 1, 256)
        hip.msda(value.view(B, n, 256), 256, offaw, offaw.shape[-1], out, B, shapes)
        torch.cuda.synchronize()
        assert _is_fence(out[B * n:])
        outs.append(out[:B * n].view(B, n, 256))
    assert _same_bits(outs[0], outs[1])
    loc, aw, z = R.msda_encoder_inputs(off, logits, shapes)
    ref, mag, spread, ix, iy, cnt = R.msda(value, shapes, loc, aw, z)
    _bounded("k_msda<%d>" % L, "%s spread %d" % (shapes, spread_logits), outs[0], ref, mag,
             _msda_chain(L), _msda_o32(value, off, logits, shapes), cond=cnt,
             extra=2 * MSDA_COORD * spread)
    # the contribution of a tap 1e4 pixels outside is exactly 0: a head all of whose taps are
    # there gives exact zeros
    far = off.clone()
    far[:, :, 5] = 1e4
    out = _nan(B * n, 256)
    hip.msda(value.view(B, n, 256), 256, _offaw(far, logits), offaw.shape[-1], out, B, shapes)
    torch.cuda.synchronize()
    assert bool((out.view(B, n, 8, 32)[:, :, 5] == 0).all())
    assert _same_bits(out.view(B, n, 8, 32)[:, :, :5], outs[0].view(B, n, 8, 32)[:, :, :5])
    if not spread_logits:                 # PN_MSDA_S3_OUT: bit for bit the split of the fp32 rows
        want = torch.zeros(hip.s3_floats(B * n, 256), device=DEV)
        hip.s3_split(outs[0].reshape(B * n, 256), want)
        got, again = torch.zeros_like(want), torch.zeros_like(want)
        hip.msda(value.view(B, n, 256), 256, offaw, offaw.shape[-1], got, B, shapes, s3_out=True)
        hip.msda(value.view(B, n, 256), 256, offaw, offaw.shape[-1], again, B, shapes, s3_out=True)
        back = _nan(B * n, 256)
        hip.s3_join(got, back)
        torch.cuda.synchronize()
        assert _same_bits(got, again) and _same_bits(got, want)
        assert _same_bits(back, outs[0].reshape(B * n, 256))


def test_fwd_msda_pixel_centres_are_exact_where_the_fp32_coordinate_is(hip):
    """On a 2 x 4 map every step of the coordinate chain is exact in fp32 (powers of two), so a tap
    planted on a pixel centre with the whole weight (logit +60 against -60: the other fifteen
    underflow to 0, the quotient is 1) returns that pixel's value rows bit for bit -- through
    pn_msda_f32 and through pn_msda_loc_f32."""
    shapes, B, h, w = [(2, 4)], 2, 2, 4
    n = h * w
    value = _d(K.msda_value(B, shapes, 77))
    off = torch.zeros(B, n, 8, 1, 4, 2, device=DEV)
    logits = torch.full((B, n, 8, 4), -60.0, device=DEV)
    want = torch.empty(B, n, 8, 32, device=DEV)
    loc = torch.zeros(B, n, 8, 1, 4, 2, device=DEV)
    aw = torch.zeros(B, n, 8, 1, 4, device=DEV)
    for tok in range(n):
        qy, qx = divmod(tok, w)
        for head in range(8):
            p, ty, tx = head % 4, (tok + head) % h, (3 * tok + head) % w
            off[:, tok, head, 0, p, 0], off[:, tok, head, 0, p, 1] = tx - qx, ty - qy
            logits[:, tok, head, p] = 60.0
            loc[:, tok, head, 0, p, 0], loc[:, tok, head, 0, p, 1] = (tx + 0.5) / w, (ty + 0.5) / h
            aw[:, tok, head, 0, p] = 1.0
            want[:, tok, head] = value[:, ty * w + tx, head]
    offaw = _offaw(off, logits)
    out = _nan(B * n, 256)
    hip.msda(value.view(B, n, 256), 256, offaw, offaw.shape[-1], out, B, shapes)
    out2 = _nan(B * n, 256)
    ss = torch.tensor(shapes, dtype=torch.int64, device=DEV)
    st = torch.zeros(1, dtype=torch.int64, device=DEV)
    hip.msda_loc(value.view(B, n, 256), 256, ss, st, loc, aw, out2, B, n, n, 1)
    torch.cuda.synchronize()
    assert torch.equal(out.view(B, n, 8, 32), want) and torch.equal(out2.view(B, n, 8, 32), want)


@pytest.mark.parametrize("Nq", [1, 3, 130])
@pytest.mark.parametrize("shapes", K.MSDA_SHAPES)
def test_fwd_msda_loc(hip, shapes, Nq):
    """pn_msda_loc_f32: explicit locations and weights.  L = 9 + levels (_msda_chain without the
    softmax); the coordinate passes MSDA_LOC_COORD roundings."""
    from oracle import layers as OL
    B, L = 2, len(shapes)
    n = sum(h * w for h, w in shapes)
    value = _d(K.msda_value(B, shapes, 11 + L))
    loc, aw = (_d(t) for t in K.msda_locations(B, shapes, Nq, 20 + Nq))
    ss = torch.tensor(shapes, dtype=torch.int64, device=DEV)
    st = torch.cat([ss.new_zeros(1), (ss[:, 0] * ss[:, 1]).cumsum(0)[:-1]])
    outs = []
    for _ in range(2):
        out = _nan(B * Nq + 1, 256)
        hip.msda_loc(value.view(B, n, 256), 256, ss, st, loc, aw, out, B, n, Nq, L)
        torch.cuda.synchronize()
        assert _is_fence(out[B * Nq:])
        outs.append(out[:B * Nq].view(B, Nq, 256))
    assert _same_bits(outs[0], outs[1])
    ref, mag, spread, ix, iy, _ = R.msda(value, shapes, loc, aw)
    _bounded("k_msda_loc<%d>" % L, "%s Nq %d" % (shapes, Nq), outs[0], ref, mag, 9 + L,
             OL.msda_core(value, shapes, loc, aw), extra=2 * MSDA_LOC_COORD * spread)


# ============================================================ fused FFN + LayerNorm
@pytest.mark.parametrize("hidden", [64, 128, 2048])
@pytest.mark.parametrize("M", [1, 31, 33, 100])
def test_fwd_ffn_ln(hip, M, hidden):
    """pn_ffn_ln_f32 / pn_ffn_ln2_f32.  With S = hidden / 64 slices, the row u = x + relu(x W1^T
    + b1) W2^T + b2 carries, relative to umag (fwd_ref.ffn_pre):
      hidden row: four 64-product quarters in parallel 64, 3 adds, + b1        = 68
      k_ffn_partial's second contraction over its 64 hidden columns            = 64
      k_reduce_ln: S - 1 adds in slice order, + b2, + x                        = S + 1
    then LayerNorm: chain = 133 + S + LN256_CHAIN, fixed = LN256_FIXED.  y2 = LayerNorm(y): its
    input rows carry y's whole bound (row maximum of L + a), on y's mag."""
    p = {k: _d(v) for k, v in K.ffn_inputs(M, hidden, M + hidden).items()}
    S = hidden // 64
    stated = hip.ffn_scratch_floats(M, hidden)
    assert stated == S * M * 256
    runs = []
    for post in (True, True, False):
        fence = _nan(stated + 128)                           # scratch of exactly the stated size
        scr = fence[64:64 + stated]
        y, y2 = _nan(M + 1, 256), _nan(M + 1, 256)
        hip.ffn_ln(p["x"], p["W1"], p["b1"], p["W2"], p["b2"], p["g"], p["b"], y[:M], scr, M, hidden,
                   post=(p["g2"], p["b2n"], y2[:M]) if post else None)
        torch.cuda.synchronize()
        assert _is_fence(fence[:64]) and _is_fence(fence[64 + stated:]), "wrote outside the scratch"
        assert _is_fence(y[M:]) and _is_fence(y2[M:]) and (post or _is_fence(y2))
        runs.append((y[:M], y2[:M]))
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])
    assert _same_bits(runs[2][0], runs[0][0]), "pn_ffn_ln_f32 differs from pn_ffn_ln2_f32's y"
    y, y2 = runs[0]
    want2 = _nan(M, 256)
    hip.layernorm(y, p["g2"], p["b2n"], want2)
    torch.cuda.synchronize()
    assert _same_bits(y2, want2), "y2 is not pn_layernorm_f32 of y"
    u, umag, h, hmag = R.ffn_pre(p["x"], p["W1"], p["b1"], p["W2"], p["b2"])
    ref, mag, amp, amp2 = R.layer_norm(u, p["g"], p["b"], 1e-5, xmag=umag)
    o32 = F.layer_norm(p["x"] + F.linear(F.relu(F.linear(p["x"], p["W1"], p["b1"])), p["W2"], p["b2"]),
                       (256,), p["g"], p["b"], 1e-5)
    case = "M %d hidden %d" % (M, hidden)
    Ly = _ln_count(133 + S + LN256_CHAIN, LN256_FIXED, amp, amp2)
    _, a = _bounded("k_ffn_partial+k_reduce_ln", case, y, ref, mag, Ly, o32)
    ref2, mag2, amp_, amp2_ = R.layer_norm(ref, p["g2"], p["b2n"], 1e-5, xmag=mag)
    chain2 = (Ly + a).amax(-1, keepdim=True) + LN256_CHAIN
    _bounded("k_reduce_ln y2", case, y2, ref2, mag2,
             chain2 * (1.0 + amp_) + chain2 * chain2 * amp2_ + LN256_FIXED,
             F.layer_norm(o32, (256,), p["g2"], p["b2n"], 1e-5))


# ============================================================ refused calls
def test_fwd_entries_refuse_malformed_calls_without_a_launch(hip):
    """Every refusal the entries document is the wrapper's "argument contract violated" (the
    entry returned PN_BAD_ARG, not a HIP error after a launch), and every buffer a call could
    have written -- outputs, scratch, partial sums, mask words -- keeps its fill bit for bit."""
    z = lambda *s: torch.zeros(*s, device=DEV)
    out = _nan(256, 256)
    scr = _nan(4096)
    out98 = _nan(4, 98)
    part = torch.full((64,), NAN, device=DEV, dtype=torch.float64)
    obits = torch.full((64,), 0x5a5a5a5a, device=DEV, dtype=torch.int32)
    orow = torch.full((32,), 7, device=DEV, dtype=torch.int32)
    q = z(64 + 1, 256)
    bits, rowall = torch.zeros(64, device=DEV, dtype=torch.int32), torch.zeros(32, device=DEV,
                                                                               dtype=torch.int32)
    att = lambda **kw: hip.attention(**{**dict(q=q[:32], ldq=256, k=q[:32], ldk=256, v=q[:32], ldv=256,
                                               bits=None, rowall=None, out=out, ldo=256, scratch=scr,
                                               B=1, Q=32, Nk=32, scale=0.2), **kw})
    bad = [
        lambda: att(ldq=258),                                        # a leading dimension % 4
        lambda: att(ldo=257),
        lambda: att(ldk=254),
        lambda: att(q=q.view(-1)[1:1 + 32 * 256].view(32, 256)),     # a misaligned pointer
        lambda: att(scratch=scr[1:]),
        lambda: att(ldk=1 << 24),                                    # Nk * ld >= 2^29
        lambda: att(ldv=1 << 24),
        lambda: att(bits=bits),                                      # bits without rowall
        lambda: att(Nk=0),
        lambda: hip.mask_pack(q[:32], obits, orow, 0, 32),
        # C not a multiple of 4, C > 3072, a misaligned row pointer
        lambda: hip.layernorm_rows(z(4, 98), z(98), z(98), out98),
        lambda: hip.layernorm_rows(z(4, 3076), z(3076), z(3076), out.view(-1)[:4 * 3076].view(4, 3076)),
        lambda: hip.layernorm_rows(z(4, 12)[:, 2:10], z(8), z(8), out[:4, :8]),
        lambda: hip.layernorm_rows_s3(z(32, 24), z(24), z(24), out.view(-1)),          # C % 16
        lambda: hip.patch_merge_ln(z(1, 4, 6), z(24), z(24), out.view(-1)[:24], 1, 2, 2, 6),
        lambda: hip.patch_merge_ln(z(1, 4, 800), z(3200), z(3200), out.view(-1)[:3200], 1, 2, 2, 800),
        # window attention: ws^2 > 169, shift >= ws, C != 32 heads, a leading dimension % 4
        lambda: hip.window_attention(z(196, 96), z(96), z(1, 27 * 27), out[:196, :32], 1, 14, 14, 32,
                                     1, 14, 0),
        lambda: hip.window_attention(z(49, 96), z(96), z(1, 169), out[:49, :32], 1, 7, 7, 32, 1, 7, 7),
        lambda: hip.window_attention(z(49, 98)[:, :96], z(96), z(1, 169), out[:49, :32], 1, 7, 7, 32,
                                     1, 7, 0),
        # group norm: a group count that does not divide into float4s, a batch stride % 4
        lambda: hip.groupnorm_nhwc(z(1, 4, 256), z(256), z(256), out[:4], part, 1, 4, 3,
                                   False, 1024, 1024),
        lambda: hip.groupnorm_nhwc(z(1, 4, 256), z(256), z(256), out[:4], part, 1, 4, 32,
                                   False, 1026, 1024),
        lambda: hip.bilinear_nhwc(z(1, 4, 6), out.view(-1)[:96], 1, 2, 2, 4, 4, 6, False, 24, 96),
        lambda: hip.bilinear_planar(z(1, 2, 2), out.view(-1), 1, 2, 2, 0, 4),
        lambda: hip.bilinear_stencil_rows(z(1, 4, 6), out.view(-1), 1, 2, 2, 2, 2, 6, 24, 96),
        # deformable sampling: ld_value < 256, more than four levels, a misaligned value pointer
        lambda: hip.msda(z(1, 4, 256), 252, z(1, 4, 96), 96, out[:4], 1, [(2, 2)]),
        lambda: hip.msda(z(1, 5, 256), 256, z(1, 5, 480), 480, out[:5], 1, [(1, 1)] * 5),
        lambda: hip.msda(z(1, 5, 256).view(-1)[1:1025], 256, z(1, 4, 96), 96, out[:4], 1, [(2, 2)]),
        lambda: hip.msda_loc(z(1, 4, 256), 256, torch.tensor([[2, 2]], device=DEV),
                             torch.zeros(1, dtype=torch.int64, device=DEV), z(1, 1, 8, 1, 4, 2),
                             z(1, 1, 8, 1, 4), out[:1], 1, 4, 0, 1),
        # fused FFN: hidden % 64, a misaligned scratch
        lambda: hip.ffn_ln(z(4, 256), z(100, 256), z(100), z(256, 100), z(256), z(256), z(256), out[:4],
                           scr, 4, 100),
        lambda: hip.ffn_ln(z(4, 256), z(64, 256), z(64), z(256, 64), z(256), z(256), z(256), out[:4],
                           scr[1:], 4, 64),
    ]
    assert len(bad) == 30
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError, match="argument contract violated"):
            call()
            pytest.fail("refusal %d was accepted" % i)
    torch.cuda.synchronize()
    assert _is_fence(out) and _is_fence(scr) and _is_fence(out98)
    assert bool(torch.isnan(part).all())
    assert bool((obits == 0x5a5a5a5a).all()) and bool((orow == 7).all())
