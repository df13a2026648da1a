"""GPU: every backward kernel of csrc/grad.hip and csrc/loss.hip, and the weight-gradient GEMM
set-up of grad.py, one at a time against a float64 statement of the same operation (torch
autograd, or an explicit matmul / unfold / fold), at the production shapes of an 800x1333
training step and at the edges where kernels of this shape go wrong: ragged chunks and slices,
odd map sizes, masks whose last 32-key word is partial, all-masked rows, strided views, tiny and
zero norms, ignored loss rows.  The composite tests (test_grad_gpu, test_losses_gpu,
test_train_gpu) run at toy sizes and compare against 1e-4 of a tensor's largest entry; these
bound every element.

Bounds.  A sum of products must satisfy |got - ref| <= c 2^-24 mag element-wise, where `mag` is
the same float64 computation on absolute values (subtractions become additions), so a dropped
or doubled term anywhere shows however small its entry.  Softmax-type kernels (attention, CE,
Seesaw) are bounded by c 2^-24 times each row's largest reference entry.  FLT_MIN is added to
every bound (exp() results below it underflow in fp32).  The c of each kernel is about 4x the
worst ratio measured on MI355X; every test prints its measured ratios.  Data-movement kernels
match bitwise.  Kernels that claim a fixed summation order are launched twice and must agree
bitwise."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
FLT_MIN = 2.0 ** -126

# c per kernel (see the module docstring): about 4x the worst ratio measured on MI355X, which
# the comment quotes with the case it came from
C_LIN = 30.0       # 7.51  dX, M = 21 950, N = 544, K = 256 (dW 2.01 at M = 100; db 0.81)
C_COLSUM = 3.0     # 0.66  1 x 1, accumulate
C_WGRAD = 14.0     # 3.44  _conv3x3_bwd 8x8, 128, stride 2 (conv_wgrad alone 2.86: 5x6, 7x7 taps)
C_DGRAD = 30.0     # 7.21  _conv3x3_bwd 200x334, 128, stride 2
C_MHA = 115.0      # 28.41 dq, B = 1, Nq = 100, Nk = 16 700
C_LN = 13.0        # 3.24  dx, 21 950 rows
C_GN = 12.0        # 2.81  gxhat, G = 32, HW = 16 700
C_COS = 17.0       # 4.17  d o, B = 2, Q = 100
C_ML = 21.0        # 5.13  mlearner_last_bwd_data, B = 2, S = 100 (tapcorr1 + colsum less)
C_OFFAW = 21.0     # 5.15  d logits, 21 950 rows, L = 3
C_CE = 14.0        # 3.41  some rows ignored, class weights
C_SEESAW = 25.0    # 6.24  cum_samples spread over 1e5, p = 0, q = 2
C_BCE = 15.0       # 3.58  random positives


@pytest.fixture(scope="module")
def hip(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip as h
    h.lib()
    return h


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * scale


def _within(name, got, ref, mag, c):
    """|got - ref| <= c 2^-24 mag + FLT_MIN element-wise; prints and returns the worst ratio."""
    got = got.detach().to(DEV).double()
    ref, mag = ref.detach().to(DEV).double(), mag.detach().to(DEV).double()
    assert got.shape == ref.shape == mag.shape, (name, got.shape, ref.shape, mag.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % name
    err = (got - ref).abs()
    ratio = (err - FLT_MIN).clamp_min(0.0) / (U * mag)
    ratio = torch.where(err <= FLT_MIN, torch.zeros_like(ratio), ratio)   # (0 / 0: exact zeros)
    worst = float(ratio.max())
    print("%-44s worst |err| / (2^-24 mag) = %9.3f   (bound %g)" % (name, worst, c))
    assert worst <= c, "%s: |err| up to %.3g x 2^-24 mag (bound %g), max |err| %.3e" % (
        name, worst, c, float(err.max()))
    return worst


def _within_rows(name, got, ref, c):
    """Softmax-type bound: |got - ref| <= c 2^-24 max |ref row| + FLT_MIN."""
    ref = ref.detach().to(DEV).double()
    return _within(name, got, ref, ref.abs().amax(-1, keepdim=True).expand_as(ref), c)


class _Tape:
    """The attributes grad.py's RelationTailGrad._lin_bwd / BackboneGrad._conv3x3_bwd read, so
    the tests run those exact call sequences on tensors of their own."""

    def __init__(self, w=None, bn_scale=None):
        import types
        from pairnet_amd.grad import RelationTailGrad
        self.dev = torch.device(DEV)
        self.head = self.backbone = types.SimpleNamespace(w=w or {})
        self.bn_scale = bn_scale or {}
        self._E = lambda *shape: RelationTailGrad._E(self, *shape)


# ============================================================ linear layers: _lin_bwd
# (contraction M, output N, input K, dy row stride, dy column offset): the pixel decoder's
# 21 950 tokens (544 = value/offset/weight projections), a masked-decoder level's 16 700 keys,
# layer2.0.conv1's 66 800 C2 pixels (200 x 334), ragged last K-slices (2080 -> 65 chunks in
# 13 slices; 21 952 and 66 816 padded rows), d_offaw's strided column blocks, and two M < 2048
# cases for the unsplit branch
LIN_CASES = [(2048, 256, 256, 256, 0), (2048, 544, 256, 544, 0), (2080, 544, 256, 544, 0),
             (2080, 128, 256, 128, 0), (2080, 512, 128, 512, 0), (21950, 544, 256, 544, 0),
             (21950, 256, 256, 256, 0), (21950, 128, 256, 128, 0), (16700, 512, 128, 512, 0),
             (66800, 128, 256, 128, 0), (66800, 512, 128, 512, 0), (66800, 544, 256, 544, 0),
             (2048, 192, 256, 288, 0), (21950, 96, 256, 288, 192), (1000, 256, 256, 256, 0),
             (100, 544, 256, 544, 0)]


@pytest.mark.parametrize("M,N,K,ld,col0", LIN_CASES)
def test_lin_bwd_weight_and_data_gradient(hip, M, N, K, ld, col0):
    """RelationTailGrad._lin_bwd as every backward class runs it: zero-padded transpose,
    split-K (16 slices, 64x64 tiles) dW GEMM from M >= 2048, add_periodic into the running
    gradient, bias colsum, dX GEMM."""
    from pairnet_amd.grad import RelationTailGrad
    g = _gen(M * 31 + N * 7 + K + col0)
    dy_full = _randn(g, M, ld)
    dy = dy_full[:, col0:col0 + N]
    x, W = _randn(g, M, K), _randn(g, N, K, scale=0.05)
    prev_w, prev_b = _randn(g, N, K), _randn(g, N)

    def run():
        grads = {"w": prev_w.clone(), "b": prev_b.clone()}
        dx = RelationTailGrad._lin_bwd(_Tape(), dy, x, W, grads, "w", "b")
        return grads["w"], grads["b"], dx

    gw, gb, dx = run()
    gw2, gb2, dx2 = run()
    torch.cuda.synchronize()
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2) and torch.equal(dx, dx2), \
        "_lin_bwd is not bitwise reproducible"
    d64, x64, W64 = dy.double(), x.double(), W.double()
    name = "lin_bwd M=%d N=%d K=%d" % (M, N, K)
    _within(name + " dW", gw, prev_w.double() + d64.T @ x64,
            prev_w.double().abs() + d64.abs().T @ x64.abs(), C_LIN)
    _within(name + " db", gb, prev_b.double() + d64.sum(0),
            prev_b.double().abs() + d64.abs().sum(0), C_LIN)
    _within(name + " dX", dx, d64 @ W64, d64.abs() @ W64.abs(), C_LIN)


# ============================================================ colsum
# (rows, cols, ld, accumulate): < 50 M elements each; 1024 rows is the first chunked launch
COLSUM_CASES = [(1, 2048, 2048, False), (1, 1, 1, True), (1023, 65, 96, False),
                (1024, 63, 64, True), (1024, 64, 64, False), (1025, 1, 4, False),
                (21950, 2048, 2048, False), (21950, 65, 288, True), (66800, 64, 80, True),
                (66800, 1, 4, False), (66800, 63, 63, False)]


@pytest.mark.parametrize("rows,cols,ld,acc", COLSUM_CASES)
def test_colsum(hip, rows, cols, ld, acc):
    g = _gen(rows * 3 + cols + ld)
    big = _randn(g, rows, ld)
    x = big[:, :cols]
    out0 = _randn(g, cols)
    out = out0.clone()
    hip.colsum(x, out, accumulate=acc)
    out2 = out0.clone()
    hip.colsum(x, out2, accumulate=acc)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    x64 = x.double()
    ref, mag = x64.sum(0), x64.abs().sum(0)
    if acc:
        ref, mag = ref + out0.double(), mag + out0.double().abs()
    _within("colsum %dx%d ld %d acc %d" % (rows, cols, ld, acc), out, ref, mag, C_COLSUM)


# ============================================================ convolution weight gradient
def _unfold_ref(dY, X, K, stride, pad):
    """dW[co][tap][ci] = sum dY[b][y][x][co] X[b][y s + kh - p][x s + kw - p][ci] in float64
    (channel-last fp32 inputs on the GPU), and the same on |dY|, |X|."""
    B, Ho, Wo, Co = dY.shape
    Ci = X.shape[3]
    outs = []
    for f in (lambda t: t, torch.abs):
        cols = F.unfold(f(X.double()).permute(0, 3, 1, 2), K, padding=pad, stride=stride)
        assert cols.shape[2] == Ho * Wo
        d = f(dY.double()).reshape(B, Ho * Wo, Co)
        w = torch.zeros(Co, Ci * K * K, dtype=torch.float64, device=DEV)
        for b in range(B):
            w += d[b].T @ cols[b].T
        outs.append(w.view(Co, Ci, K * K).permute(0, 2, 1).contiguous())
    return outs


# (B, Hi, Wi, Ci, Co, K, stride, pad, rows_per): rows_per that does not divide Ho, odd and
# even maps, K in {1, 3, 7}, padding wider than K / 2; the Matrix Learner's 64 -> 64 7x7 at
# S = 100, rows_per = 10 as grad.py runs it (the backbone's production 3x3 layers are below,
# through _conv3x3_bwd)
WGRAD_CASES = [(2, 13, 10, 64, 256, 1, 2, 0, 3), (2, 9, 11, 256, 64, 3, 1, 0, 4),
               (2, 7, 7, 64, 128, 3, 2, 1, 3), (2, 15, 16, 64, 64, 7, 2, 3, 3),
               (2, 5, 6, 128, 64, 7, 1, 3, 2), (2, 8, 9, 64, 64, 3, 2, 3, 5),
               (1, 1, 1, 64, 64, 3, 1, 1, 1), (2, 100, 100, 64, 64, 7, 1, 3, 10)]


@pytest.mark.parametrize("B,Hi,Wi,Ci,Co,K,stride,pad,rows_per", WGRAD_CASES)
def test_conv_wgrad_over_chunks(hip, B, Hi, Wi, Ci, Co, K, stride, pad, rows_per):
    Ho, Wo = (Hi + 2 * pad - K) // stride + 1, (Wi + 2 * pad - K) // stride + 1
    g = _gen(Hi * 1000 + Wi * 10 + K + Ci + Co + stride)
    X, dY = _randn(g, B, Hi, Wi, Ci), _randn(g, B, Ho, Wo, Co)
    chunks = B * ((Ho + rows_per - 1) // rows_per)

    def run():
        part = torch.full((chunks, Co * K * K * Ci), float("nan"), device=DEV)
        hip.conv_wgrad(dY, X, part, B, Hi, Wi, Ho, Wo, Ci, Co, K, stride, pad, rows_per)
        dw = torch.empty(Co * K * K * Ci, device=DEV)
        hip.colsum(part, dw)
        return dw

    dw, dw2 = run(), run()
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2), "conv_wgrad + colsum is not bitwise reproducible"
    ref, mag = _unfold_ref(dY, X, K, stride, pad)
    _within("conv_wgrad %dx%d %d->%d K%d s%d p%d rows %d" % (Hi, Wi, Ci, Co, K, stride, pad,
                                                           rows_per),
            dw.view(Co, K * K, Ci), ref, mag, C_WGRAD)


# ============================================================ _conv3x3_bwd (weight + data)
def _fold_ref(dY, Wt, Hi, Wi, stride):
    """d X of a 3x3 pad-1 convolution (Wt [Co][Ci][3][3] float64) via fold, and on |.|."""
    B, Ho, Wo, Co = dY.shape
    outs = []
    for f in (lambda t: t, torch.abs):
        Wm = f(Wt).reshape(Co, -1)
        d = f(dY.double()).reshape(B, Ho * Wo, Co)
        cols = torch.stack([Wm.T @ d[b].T for b in range(B)])          # [B][Ci*9][L]
        dx = F.fold(cols, (Hi, Wi), 3, padding=1, stride=stride)
        outs.append(dx.permute(0, 2, 3, 1))
    return outs


# (B, hi, wi, planes, stride): the backbone's 3x3 layers at 800x1333 (layer2 at C2 200x334,
# layer3, layer4; stride-2 input widths 334 and the odd 167 and 84), and small odd / even maps
CONV3_CASES = [(2, 200, 334, 128, 2), (2, 100, 167, 128, 1), (2, 100, 167, 256, 2),
               (2, 50, 84, 256, 1), (2, 50, 84, 512, 2), (2, 25, 42, 512, 1),
               (2, 9, 12, 64, 2), (2, 10, 11, 64, 2), (2, 7, 7, 64, 2), (2, 8, 8, 128, 2),
               (2, 9, 13, 64, 1), (1, 3, 2, 64, 2)]


@pytest.mark.parametrize("B,hi,wi,planes,stride", CONV3_CASES)
def test_conv3x3_bwd_weight_and_data_gradient(hip, B, hi, wi, planes, stride):
    """BackboneGrad._conv3x3_bwd: conv_wgrad in chunks of min(h, 8) output rows + colsum +
    scale_rows for d weight; conv_weight_bwd_layout (+ dilate2 at stride 2) + conv2d_ex for
    d input."""
    from pairnet_amd.grad import BackboneGrad
    h, wd = (hi - 1) // stride + 1, (wi - 1) // stride + 1
    g = _gen(hi * 997 + wi + planes + stride)
    t1 = _randn(g, B, hi, wi, planes)
    d_t2 = _randn(g, B, h, wd, planes)
    Wt = _randn(g, planes, planes, 3, 3, scale=0.05)
    bn = torch.rand(planes, generator=g, device=DEV) + 0.5
    p = "layerX.0."
    tape = _Tape(w={p + "conv2.w": Wt.permute(0, 2, 3, 1).contiguous()},
                 bn_scale={p + "conv2.weight": bn})
    s = dict(p=p, planes=planes, stride=stride, hi=hi, wi=wi, h=h, w=wd, t1=t1)

    def run():
        grads = {p + "conv2.weight": torch.empty(planes, planes, 3, 3, device=DEV)}
        d_t1 = BackboneGrad._conv3x3_bwd(tape, s, d_t2, grads, B)
        return grads[p + "conv2.weight"], d_t1

    gw, d_t1 = run()
    gw2, d_t12 = run()
    torch.cuda.synchronize()
    assert torch.equal(gw, gw2) and torch.equal(d_t1, d_t12)
    name = "conv3x3_bwd %dx%d %d s%d" % (hi, wi, planes, stride)
    ref, mag = _unfold_ref(d_t2, t1, 3, stride, 1)                   # [co][tap][ci]
    sc = bn.double()[:, None, None]
    _within(name + " dW", gw.permute(0, 2, 3, 1).reshape(planes, 9, planes), ref * sc, mag * sc,
            C_WGRAD)
    ref, mag = _fold_ref(d_t2, Wt.double(), hi, wi, stride)
    _within(name + " dX", d_t1, ref, mag, C_DGRAD)


# ============================================================ data movement: bitwise
@pytest.mark.parametrize("B,Hi,Wi,Ho,Wo,C", [(2, 9, 12, 5, 6, 64), (2, 10, 11, 5, 6, 2048),
                                             (1, 7, 7, 4, 4, 64), (2, 8, 8, 4, 4, 64),
                                             (2, 9, 9, 3, 2, 64), (1, 1, 1, 1, 1, 2048)])
def test_dilate2_and_subsample2_bitwise(hip, B, Hi, Wi, Ho, Wo, C):
    g = _gen(Hi * 100 + Wi + C)
    x = _randn(g, B, Ho, Wo, C)
    want = torch.zeros(B, Hi, Wi, C, device=DEV)
    want[:, 0:2 * Ho:2, 0:2 * Wo:2] = x
    out = torch.full((B, Hi, Wi, C), float("nan"), device=DEV)
    hip.dilate2(x, out, B, Hi, Wi, Ho, Wo, C)
    base = _randn(g, B, Hi, Wi, C)
    acc = base.clone()
    hip.dilate2(x, acc, B, Hi, Wi, Ho, Wo, C, accumulate=True)
    big = _randn(g, B, Hi, Wi, C)
    sub = torch.full((B, Ho, Wo, C), float("nan"), device=DEV)
    hip.subsample2(big, sub, B, Hi, Wi, Ho, Wo, C)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(acc, base + want)
    assert torch.equal(sub, big[:, 0:2 * Ho:2, 0:2 * Wo:2])


@pytest.mark.parametrize("Co,T,Ci", [(64, 9, 64), (64, 49, 64), (64, 49, 1), (2048, 1, 64),
                                     (64, 1, 2048), (37, 9, 5)])
def test_conv_weight_bwd_layout_bitwise(hip, Co, T, Ci):
    w = _randn(_gen(Co * T * Ci), Co, T, Ci)
    out = torch.full((Ci, T, Co), float("nan"), device=DEV)
    hip.conv_weight_bwd_layout(w, out, Co, T, Ci)
    torch.cuda.synchronize()
    assert torch.equal(out, w.flip(1).permute(2, 1, 0))


@pytest.mark.parametrize("rows,cols", [(64, 576), (2048, 1), (1, 2048), (3, 5), (512, 4608)])
def test_scale_rows_bitwise(hip, rows, cols):
    g = _gen(rows * 7 + cols)
    x, s = _randn(g, rows, cols), _randn(g, rows)
    y = x.clone()
    hip.scale_rows(y, s)
    torch.cuda.synchronize()
    assert torch.equal(y, x * s[:, None])


# ============================================================ attention backward
def _mha_ref(q, k, v, do, B, Nq, Nk, scale, allowed):
    """float64 autograd of softmax(scale q k^T, masked) v per 8 heads x 32 (2-D fp32 views)."""
    hd = lambda t, n: t.contiguous().double().view(B, n, 8, 32).transpose(1, 2) \
        .detach().requires_grad_()
    q64, k64, v64 = hd(q, Nq), hd(k, Nk), hd(v, Nk)
    s = scale * (q64 @ k64.transpose(-1, -2))
    if allowed is not None:
        s = s.masked_fill(~allowed[:, None], float("-inf"))
    o = torch.softmax(s, -1) @ v64
    o.backward(do.contiguous().double().view(B, Nq, 8, 32).transpose(1, 2))
    back = lambda t, n: t.grad.transpose(1, 2).reshape(B * n, 256)
    return back(q64, Nq), back(k64, Nk), back(v64, Nk)


# (B, Nq, Nk, masked): the masked decoder's three levels at 800x1333 (Nk not a multiple of 32:
# a partial last mask word), Nq not a multiple of 8, and the single-key edge
MHA_CASES = [(1, 100, 16700, True), (2, 100, 4200, True), (2, 37, 1050, True),
             (2, 13, 70, True), (1, 1, 1, False), (2, 9, 33, False)]


@pytest.mark.parametrize("B,Nq,Nk,masked", MHA_CASES)
def test_mha_bwd(hip, B, Nq, Nk, masked):
    g = _gen(B * 100000 + Nq * 1000 + Nk)
    q, k, v = _randn(g, B * Nq, 256), _randn(g, B * Nk, 256), _randn(g, B * Nk, 256)
    do = _randn(g, B * Nq, 256)
    bits = rowall = allowed = None
    if masked:
        logits = _randn(g, B * Nq, Nk)
        logits[::5] = -logits[::5].abs() - 0.5              # every 5th row: all keys masked
        logits[1, :] = -1.0
        logits[1, -1] = 1.0                                  # only the very last key attendable
        bits = torch.empty(B * Nq, (Nk + 31) // 32, dtype=torch.int32, device=DEV)
        rowall = torch.empty(B * Nq, dtype=torch.int32, device=DEV)
        hip.mask_pack(logits, bits, rowall, B * Nq, Nk)
        m = logits < 0
        allowed = (~m | m.all(-1, keepdim=True)).view(B, Nq, Nk)
    scale = 32 ** -0.5
    scr = torch.empty(hip.mha_bwd_scratch_floats(B, Nq, Nk), device=DEV)

    def run():
        dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
        hip.mha_bwd(q, k, v, do, dq, dk, dv, scr, B, Nq, Nk, scale, bits=bits, rowall=rowall)
        return dq, dk, dv

    got, got2 = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, got2)), "mha_bwd is not reproducible"
    if masked:
        assert int(rowall.sum()) >= (B * Nq + 4) // 5
    refs = _mha_ref(q, k, v, do, B, Nq, Nk, scale, allowed)
    for nm, a, r in zip(("dq", "dk", "dv"), got, refs):
        _within_rows("mha_bwd B%d Nq%d Nk%d %s" % (B, Nq, Nk, nm), a, r, C_MHA)


def test_mha_bwd_self_attention_on_packed_qkv(hip):
    """grad.py's self-attention: q / k / v and dq / dk / dv are column blocks of [Q|K|V] rows
    (row stride 768)."""
    B, N = 2, 200
    g = _gen(768)
    QKV, do = _randn(g, B * N, 768), _randn(g, B * N, 256)
    scr = torch.empty(hip.mha_bwd_scratch_floats(B, N, N), device=DEV)
    dQKV = torch.full((B * N, 768), float("nan"), device=DEV)
    hip.mha_bwd(QKV, QKV[:, 256:], QKV[:, 512:], do, dQKV, dQKV[:, 256:], dQKV[:, 512:], scr,
                B, N, N, 32 ** -0.5)
    torch.cuda.synchronize()
    refs = _mha_ref(QKV[:, :256], QKV[:, 256:512], QKV[:, 512:], do, B, N, N, 32 ** -0.5, None)
    for j, (nm, r) in enumerate(zip(("dq", "dk", "dv"), refs)):
        _within_rows("mha_bwd packed QKV %s" % nm, dQKV[:, 256 * j:256 * (j + 1)], r, C_MHA)


# ============================================================ LayerNorm(256) backward
def _norm_mag(x64, g64, dims, rstd):
    """|.|-magnitude of dx = rstd (g - mean g - xhat mean(g xhat)) over `dims` (xhat's
    centring counted as |x| + mean |x|)."""
    axh = (x64.abs() + x64.abs().mean(dims, keepdim=True)) * rstd
    return rstd * (g64.abs() + g64.abs().mean(dims, keepdim=True)
                   + axh * (g64.abs() * axh).mean(dims, keepdim=True)), axh


@pytest.mark.parametrize("rows,offset", [(1, 0.0), (3, 0.0), (21950, 0.0), (3, 1e3),
                                         (21950, 1e3)])
def test_layernorm256_bwd(hip, rows, offset):
    g = _gen(rows + int(offset))
    x = _randn(g, rows, 256) + offset
    dy, gam, bet = _randn(g, rows, 256), _randn(g, 256), _randn(g, 256)
    dx, gx = torch.empty_like(x), torch.empty_like(x)
    hip.layernorm256_bwd(dy, x, gam, dx, gx)
    dgam, dbet = torch.empty(256, device=DEV), torch.empty(256, device=DEV)
    hip.colsum(gx, dgam)
    hip.colsum(dy, dbet)
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_()
    g64, b64 = gam.double().requires_grad_(), bet.double().requires_grad_()
    F.layer_norm(x64, (256,), g64, b64, 1e-5).backward(dy.double())
    xd = x64.detach()
    rstd = 1.0 / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + 1e-5)
    xhat = (xd - xd.mean(-1, keepdim=True)) * rstd
    gg = dy.double() * gam.double()
    mag, axh = _norm_mag(xd, gg, -1, rstd)
    name = "layernorm256_bwd rows %d offset %g" % (rows, offset)
    _within(name + " dx", dx, x64.grad, mag, C_LN)
    _within(name + " gxhat", gx, dy.double() * xhat, dy.double().abs() * axh, C_LN)
    _within(name + " dgamma", dgam, g64.grad, (dy.double().abs() * axh).sum(0), C_LN)
    _within(name + " dbeta", dbet, b64.grad, dy.double().abs().sum(0), C_LN)


# ============================================================ GroupNorm backward (channel-last)
@pytest.mark.parametrize("G,HW", [(32, 16700), (32, 1050), (32, 7), (1, 1050), (1, 1),
                                  (256, 7), (256, 1), (256, 4200)])
def test_groupnorm_nhwc_bwd(hip, G, HW):
    """grad.py's pixel-decoder call: x a [B][HW][256] map, dy a level's rows inside the
    [B][SN][256] token gradient (dy_bstride != x_bstride, offset base)."""
    B, extra, off = 2, 37, 5
    g = _gen(G * 100000 + HW)
    x = _randn(g, B, HW, 256, scale=2.0) + 0.5
    dy_big = _randn(g, B, HW + extra, 256)
    dy = dy_big[:, off:off + HW]
    gam = _randn(g, 256)
    stats = torch.empty(B * G * 4, device=DEV)

    def run():
        dx, gx = torch.empty(B * HW, 256, device=DEV), torch.empty(B * HW, 256, device=DEV)
        hip.groupnorm_nhwc_bwd(x, dy, gam, dx, gx, stats, B, HW, G, HW * 256,
                               (HW + extra) * 256)
        dgam, dbet = torch.zeros(256, device=DEV), torch.zeros(256, device=DEV)
        hip.colsum(gx, dgam, accumulate=True)
        for b in range(B):
            hip.colsum(dy[b], dbet, accumulate=True)
        return dx, gx, dgam, dbet

    got, got2 = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, got2)), "groupnorm_nhwc_bwd not reproducible"
    dx, gx, dgam, dbet = got
    x64 = x.double().permute(0, 2, 1).contiguous().requires_grad_()          # [B][256][HW]
    g64 = gam.double().requires_grad_()
    b64 = torch.zeros(256, dtype=torch.float64, device=DEV, requires_grad=True)
    d64 = dy.double().permute(0, 2, 1)
    F.group_norm(x64, G, g64, b64, 1e-5).backward(d64)
    cpg = 256 // G
    xg = x.double().view(B, HW, G, cpg)
    mean = xg.mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(((xg - mean) ** 2).mean((1, 3), keepdim=True) + 1e-5)
    xhat = ((xg - mean) * rstd).view(B, HW, 256)
    gg = (dy.double() * gam.double()).view(B, HW, G, cpg)
    mag, axh = _norm_mag(xg, gg, (1, 3), rstd)
    axh = axh.view(B, HW, 256)
    name = "groupnorm_nhwc_bwd G %d HW %d" % (G, HW)
    _within(name + " dx", dx.view(B, HW, 256), x64.grad.permute(0, 2, 1), mag.view(B, HW, 256),
            C_GN)
    _within(name + " gxhat", gx.view(B, HW, 256), dy.double() * xhat, dy.double().abs() * axh,
            C_GN)
    _within(name + " dgamma", dgam, g64.grad, (dy.double().abs() * axh).sum((0, 1)), C_GN)
    _within(name + " dbeta", dbet, b64.grad, dy.double().abs().sum((0, 1)), C_GN)


# ============================================================ cosine block backward
@pytest.mark.parametrize("B,Q", [(1, 1), (2, 37), (2, 100), (1, 100)])
def test_cosine_bwd(hip, B, Q):
    """Both sides of raw = normalize(s) normalize(o)^T (eps 1e-12) for a non-symmetric d raw;
    one all-zero row and one row of norm 0.5e-12 (below eps: F.normalize divides by eps)."""
    g = _gen(B * 1000 + Q)
    s, o = _randn(g, B, Q, 256), _randn(g, B, Q, 256)
    draw = _randn(g, B, Q, Q)
    if Q >= 3:
        for t, r in ((s, 0), (o, Q - 1)):
            t[-1, r] = 0.0
            tiny = _randn(g, 256)
            t[0, r + (1 if r == 0 else -1)] = tiny * (0.5e-12 / float(tiny.norm()))
    s64, o64 = s.double().requires_grad_(), o.double().requires_grad_()
    sh, oh = F.normalize(s64, dim=-1, eps=1e-12), F.normalize(o64, dim=-1, eps=1e-12)
    (sh @ oh.transpose(1, 2)).backward(draw.double())
    ds, do = torch.empty_like(s), torch.empty_like(o)
    hip.cosine_bwd(draw, s, oh.detach().float().contiguous(), ds, B, Q, False)
    hip.cosine_bwd(draw, o, sh.detach().float().contiguous(), do, B, Q, True)
    torch.cuda.synchronize()
    ad = draw.double().abs()
    for nm, x, other, a, ref, got in (("s", s, oh, ad, s64.grad, ds),
                                      ("o", o, sh, ad.transpose(1, 2), o64.grad, do)):
        x64 = x.double()
        den = x64.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        hat = x64 / den
        ag = a @ other.detach().abs()
        mag = (ag + hat.abs() * (hat.abs() * ag).sum(-1, keepdim=True)) / den
        _within("cosine_bwd B%d Q%d d%s" % (B, Q, nm), got, ref, mag, C_COS)


# ============================================================ Matrix Learner first / last layer
@pytest.mark.parametrize("B,S", [(1, 1), (2, 5), (1, 7), (2, 37), (2, 100)])
def test_mlearner_last_bwd_data_and_tapcorr1(hip, B, S):
    """The 7x7 64 -> 1 last layer (data gradient through its input ReLU, weight gradient:
    tapcorr1 sgn -1 + colsum) and the 1 -> 64 first layer's weight gradient (sgn +1), against
    float64 autograd of the convolutions (CPU)."""
    g = _gen(B * 1000 + S)
    pre = _randn(g, B, S, S, 64)
    c2 = torch.relu(pre)
    gimp = _randn(g, B, S, S)
    w3 = _randn(g, 49, 64, scale=0.1)
    dc1 = torch.relu(_randn(g, B, S, S, 64))                  # a pre-ReLU gradient with zeros
    raw = _randn(g, B, S, S)
    dc = torch.empty(B, S, S, 64, device=DEV)
    hip.mlearner_last_bwd_data(gimp, w3, c2, dc, B, S)
    part = torch.empty(B * S, 49 * 64, device=DEV)
    hip.tapcorr1(c2, gimp, part, B, S, -1)
    dw3 = torch.empty(49 * 64, device=DEV)
    hip.colsum(part, dw3)
    hip.tapcorr1(dc1, raw, part, B, S, +1)
    dw1 = torch.empty(49 * 64, device=DEV)
    hip.colsum(part, dw1)
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu().double()
    nchw = lambda t: cpu(t).permute(0, 3, 1, 2).contiguous()
    W3 = cpu(w3).t().reshape(1, 64, 7, 7).contiguous()
    p64, W3g = nchw(pre).requires_grad_(), W3.clone().requires_grad_()
    F.conv2d(torch.relu(p64), W3g, padding=3).backward(cpu(gimp)[:, None])
    gi = torch.nn.grad
    mag_dc = gi.conv2d_input(p64.shape, W3.abs(), cpu(gimp).abs()[:, None], padding=3) \
        * (p64.detach() > 0)
    mag_w3 = gi.conv2d_weight(nchw(c2).abs(), W3.shape, cpu(gimp).abs()[:, None], padding=3)
    name = "mlearner B%d S%d" % (B, S)
    _within(name + " last_bwd_data", dc.permute(0, 3, 1, 2), p64.grad, mag_dc, C_ML)
    _within(name + " tapcorr1(-1) dw3", dw3.view(49, 64).t().reshape(1, 64, 7, 7), W3g.grad,
            mag_w3, C_ML)
    ref_w1 = gi.conv2d_weight(cpu(raw)[:, None], (64, 1, 7, 7), nchw(dc1), padding=3)
    mag_w1 = gi.conv2d_weight(cpu(raw).abs()[:, None], (64, 1, 7, 7), nchw(dc1).abs(), padding=3)
    _within(name + " tapcorr1(+1) dw1", dw1.view(49, 64).t().reshape(64, 1, 7, 7), ref_w1, mag_w1,
            C_ML)


# ============================================================ MSDA offsets / weights backward
# (rows, level shapes (h, w), row stride): the pixel decoder at 800x1333 (3 levels, 21 950
# tokens), 1 and 4 levels, strides above 8 L 12, row counts off the 32-row workgroup
OFFAW_CASES = [(21950, ((100, 167), (50, 84), (25, 42)), 288),
               (37, ((13, 29),), 100), (1, ((7, 11), (5, 3), (2, 9), (1, 4)), 400),
               (1000, ((7, 11), (5, 3), (2, 9), (1, 4)), 384),
               (33, ((16, 9), (8, 5), (4, 3)), 300)]


@pytest.mark.parametrize("rows,shapes,ld", OFFAW_CASES)
def test_msda_offaw_bwd(hip, rows, shapes, ld):
    L = len(shapes)
    LP = L * 4
    g = _gen(rows * 10 + L + ld)
    gl, ga = _randn(g, rows, 8, L, 4, 2), _randn(g, rows, 8, LP)
    off64 = torch.zeros(rows, 8, L, 4, 2, dtype=torch.float64, device=DEV, requires_grad=True)
    lg64 = _randn(g, rows, 8, LP).double().requires_grad_()
    aw64 = torch.softmax(lg64, -1)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64, device=DEV)
    loc = 0.5 + off64 / norm[None, None, :, None, :]
    ((loc * gl.double()).sum() + (aw64 * ga.double()).sum()).backward()
    aw = aw64.detach().float().contiguous()
    d_offaw = _randn(g, rows, ld)
    sentinel = d_offaw[:, 8 * L * 12:].clone()
    hip.msda_offaw_bwd(gl.contiguous(), ga.contiguous(), aw, d_offaw[:, :], shapes)
    torch.cuda.synchronize()
    assert torch.equal(d_offaw[:, 8 * L * 12:], sentinel), "wrote past the row's 8 L 12 columns"
    name = "msda_offaw_bwd rows %d L %d" % (rows, L)
    _within(name + " d offsets", d_offaw[:, :8 * LP * 2].view(rows, 8, L, 4, 2), off64.grad,
            gl.double().abs() / norm[None, None, :, None, :], C_OFFAW)
    a = aw.double()
    mag = a * (ga.double().abs() + (a * ga.double().abs()).sum(-1, keepdim=True))
    _within(name + " d logits", d_offaw[:, 8 * LP * 2:8 * LP * 3].view(rows, 8, LP), lg64.grad,
            mag, C_OFFAW)


# ============================================================ loss gradients
def _targets(g, rows, C, ignore):
    t = torch.randint(0, C, (rows,), generator=g, device=DEV)
    if ignore == "some":
        t[::3] = -1
    elif ignore == "all":
        t[:] = -1
    return t


@pytest.mark.parametrize("ignore", ["none", "some", "all"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("big", [False, True])
def test_ce_mean_grad(hip, ignore, weighted, big):
    from oracle import mmdet_train as T
    rows, C, lw = 200, 134, 2.0
    g = _gen(rows + C + weighted * 7 + big * 13 + len(ignore))
    x = _randn(g, rows, C, scale=3.0)
    if big:                                                  # logits at +-80
        x[::2, 5] = 80.0
        x[1::4, :] = -80.0
        x[1::4, 7] = 80.0
    t = _targets(g, rows, C, ignore)
    cw = (torch.rand(C, generator=g, device=DEV) + 0.5) if weighted else None
    grad = torch.full((rows, C), float("nan"), device=DEV)
    hip.ce_mean_grad(x, t, cw, grad, lw)
    torch.cuda.synchronize()
    kept = t >= 0
    assert bool((grad[~kept] == 0).all()), "ignored rows must get exact zeros"
    if not bool(kept.any()):
        return
    x64 = x.double().requires_grad_()
    loss = lw * T.cross_entropy(x64[kept], t[kept], class_weight=None if cw is None else
                                cw.double())
    loss.backward()
    _within_rows("ce_mean_grad ignore %s cw %d big %d" % (ignore, weighted, big), grad[kept],
                 x64.grad[kept], C_CE)


@pytest.mark.parametrize("cum_kind", ["zeros", "spread"])
@pytest.mark.parametrize("p,q", [(0.8, 2.0), (0.0, 2.0), (0.8, 0.0), (0.0, 0.0)])
def test_seesaw_mean_grad(hip, cum_kind, p, q):
    from oracle import mmdet_train as T
    rows, C, lw, eps = 200, 57, 1.0, 1e-2
    g = _gen(rows + int(p * 10) + int(q * 100) + len(cum_kind))
    x = _randn(g, rows, C, scale=2.0)
    t = _targets(g, rows, C, "some")
    t[2], t[4] = 3, 5
    x[4] = 5.0
    x[4, 5] = -10.0                            # a row whose target score is far below eps
    if cum_kind == "zeros":
        cum = torch.randint(0, 50, (C,), generator=g, device=DEV).float()
        cum[:8] = 0.0                           # (clamped to 1 by the reference)
        t[::7] = torch.arange(rows, device=DEV)[::7] % 8
    else:
        cum = torch.pow(10.0, torch.rand(C, generator=g, device=DEV) * 5.0).round()
    grad = torch.full((rows, C), float("nan"), device=DEV)
    hip.seesaw_mean_grad(x, t, cum, grad, p, q, eps, lw)
    torch.cuda.synchronize()
    kept = t >= 0
    assert bool((grad[~kept] == 0).all()), "ignored rows must get exact zeros"
    x64 = x.double().requires_grad_()
    loss = lw * T.seesaw_ce_loss(x64[kept], t[kept], None, cum.double(), C, p, q, eps)
    loss.backward()
    _within_rows("seesaw_mean_grad cum %s p %g q %g" % (cum_kind, p, q), grad[kept],
                 x64.grad[kept], C_SEESAW)


@pytest.mark.parametrize("pos", ["one", "all", "random"])
@pytest.mark.parametrize("big", [False, True])
def test_bce_posw_mean_grad(hip, pos, big):
    B, Q, lw = 2, 100, 5.0
    n = B * Q * Q
    g = _gen(n + len(pos) + big)
    x = _randn(g, B, Q, Q, scale=3.0)
    if big:                                               # logits at +-100
        x.view(-1)[::3] = 100.0
        x.view(-1)[1::3] = -100.0
    t = torch.zeros(B, Q, Q, device=DEV)
    if pos == "one":
        t[1, 17, 42] = 1.0
    elif pos == "all":
        t[:] = 1.0
    else:
        t = (torch.rand(B, Q, Q, generator=g, device=DEV) < 0.05).float()
    grad = torch.full_like(x, float("nan"))
    hip.bce_posw_mean_grad(x, t, grad, lw)
    torch.cuda.synchronize()
    x64, t64 = x.double().requires_grad_(), t.double()
    pw = torch.tensor(float(n) / float(t64.gt(0).sum()), dtype=torch.float64, device=DEV)
    (lw * F.binary_cross_entropy_with_logits(x64, t64, pos_weight=pw, reduction="mean")).backward()
    mag = lw / n * ((1 - t64) + (1 + (pw - 1) * t64) * torch.sigmoid(-x64.detach()))
    _within("bce_posw_mean_grad pos %s big %d" % (pos, big), grad, x64.grad, mag, C_BCE)


# ============================================================ refusals
def test_backward_kernels_refuse_what_they_cannot_run(hip):
    """The C ABI refuses (RuntimeError, nothing written) what its kernels cannot run."""
    z = lambda *s: torch.zeros(*s, device=DEV)
    # conv_wgrad: Ci / Co not a multiple of 64, K > 7
    for Ci, Co, K in ((96, 64, 3), (64, 32, 3), (64, 64, 9)):
        part = torch.full((Co * K * K * Ci,), 7.0, device=DEV)
        with pytest.raises(RuntimeError):
            hip.conv_wgrad(z(1, 1, 1, Co), z(1, K, K, Ci), part, 1, K, K, 1, 1, Ci, Co, K, 1, 0, 1)
        assert bool((part == 7.0).all())
    # tapcorr1: sgn not +-1
    for sgn in (0, 2, -3):
        with pytest.raises(RuntimeError):
            hip.tapcorr1(z(1, 3, 3, 64), z(1, 3, 3), z(3, 49 * 64), 1, 3, sgn)
    # dilate2 / subsample2: Ho, Wo too large for Hi, Wi
    with pytest.raises(RuntimeError):
        hip.dilate2(z(1, 5, 4, 8), z(1, 8, 8, 8), 1, 8, 8, 5, 4, 8)
    with pytest.raises(RuntimeError):
        hip.dilate2(z(1, 4, 5, 8), z(1, 8, 8, 8), 1, 8, 8, 4, 5, 8, accumulate=True)
    with pytest.raises(RuntimeError):
        hip.subsample2(z(1, 8, 8, 8), z(1, 5, 4, 8), 1, 8, 8, 5, 4, 8)
    with pytest.raises(RuntimeError):
        hip.subsample2(z(1, 7, 7, 8), z(1, 4, 5, 8), 1, 7, 7, 4, 5, 8)
    # msda_offaw_bwd: L > 4, row stride below 8 L 12
    shapes5 = [(4, 4)] * 5
    with pytest.raises(RuntimeError):
        hip.msda_offaw_bwd(z(3, 8 * 20 * 2), z(3, 8 * 20), z(3, 8 * 20), z(3, 480), shapes5)
    d = torch.full((3, 95), 7.0, device=DEV)
    with pytest.raises(RuntimeError):
        hip.msda_offaw_bwd(z(3, 64), z(3, 32), z(3, 32), d, [(4, 4)])
    assert bool((d == 7.0).all())
    # mha_bwd: a row stride not a multiple of 4; a base pointer not 16-byte aligned
    B, Nq, Nk = 1, 8, 8
    scr = z(hip.mha_bwd_scratch_floats(B, Nq, Nk))
    k, v, do = z(Nk, 256), z(Nk, 256), z(Nq, 256)
    dq, dk, dv = (torch.full((n, 256), 7.0, device=DEV) for n in (Nq, Nk, Nk))
    for q in (z(Nq, 257)[:, :256], z(Nq, 260)[:, 1:257]):
        with pytest.raises(RuntimeError):
            hip.mha_bwd(q, k, v, do, dq, dk, dv, scr, B, Nq, Nk, 1.0)
    with pytest.raises(RuntimeError):
        hip.mha_bwd(z(Nq, 256), z(Nk, 260)[:, 2:258], v, do, dq, dk, dv, scr, B, Nq, Nk, 1.0)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (dq, dk, dv))
