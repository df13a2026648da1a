"""float64 statements of the kernels that do nearly all the arithmetic of a step: the dense
contraction pn_gemm_f32 / pn_gemm_group_f32 (csrc/gemm.hip), the implicit-GEMM convolution
pn_conv2d_nhwc_ex_f32, the stem pn_stem7x7s2_f32 (csrc/stem.hip), pn_maxpool3x3s2_nhwc_f32
(csrc/resize.hip), the Matrix Learner's edge layers pn_mlearner_first_f32 / pn_mlearner_last_f32
(csrc/ppn.hip) and the Winograd transforms (csrc/winograd.hip), written from the formulas in
include/pairnet_hip.h.  Each returns the value and `mag`, the same computation on absolute values.
tests/test_mm_refs.py pins every statement to torch in float64 (1e-12); tests/test_mm_kernels_gpu.py
compares the kernels with them, bit for bit on integer operands and element-wise under a rounding
count on random ones.  Inputs are fp32 tensors; all arithmetic is float64."""
import torch

EXACT = 2.0 ** 24     # integers below it, and their sums, are exact in fp32 in any order


def _epilogue(acc, accm, bias, res, relu, relu_after):
    """[relu_after](act(acc + bias) + res) and its mag (ReLU is 1-Lipschitz: it keeps the bound
    of its argument with its argument's mag)."""
    if bias is not None:
        acc, accm = acc + bias.double(), accm + bias.double().abs()
    if relu:
        acc = acc.clamp_min(0.0)
    if res is not None:
        acc, accm = acc + res.double(), accm + res.double().abs()
    if relu_after:
        acc = acc.clamp_min(0.0)
    return acc, accm


# ------------------------------------------------------------------------------ dense contraction
def gemm(A, W, bias=None, res=None, aadd=None, aadd_from_col=0, relu=False, relu_after=False):
    """C[z][m][n] = [relu_after](act(sum_k (A[z][m][k] + Aadd[m % rows][k]) W[z][n][k] + bias[n])
    + Res[z][m][n]) for A [Z][M][K], W [Z][N][K] (or [N][K]: shared) -> (C, mag).  Aadd feeds the
    output columns >= aadd_from_col only.  mag: sum (|A| + |Aadd|) |W| + |bias| + |Res|."""
    A64, W64 = A.double(), W.double()
    if W64.dim() == 2:
        W64 = W64.expand(A64.shape[0], -1, -1)
    Z, M, K = A64.shape
    N = W64.shape[1]
    C = torch.zeros(Z, M, N, dtype=torch.float64)
    Cm = torch.zeros(Z, M, N, dtype=torch.float64)
    add = None
    if aadd is not None:
        add = aadd.double()[torch.arange(M) % aadd.shape[0]]              # [M][K]
    for k in range(K):                    # (a loop: no BLAS call decides the order or the precision)
        a = A64[:, :, k, None]
        w = W64[:, None, :, k]
        C += a * w
        Cm += a.abs() * w.abs()
        if add is not None:
            sel = (torch.arange(N) >= aadd_from_col).double()[None, None, :]
            C += add[None, :, k, None] * w * sel
            Cm += add[None, :, k, None].abs() * w.abs() * sel
    return _epilogue(C, Cm, bias, res, relu, relu_after)


# ------------------------------------------------------------------------------ convolution
def conv2d(x, w, bias=None, res=None, stride=1, pad=0, relu=False, relu_after=False):
    """Channel-last convolution: x [B][H][W][Cin], w [Cout][Cin][KH][KW] (torch's layout),
    res / out [B][Ho][Wo][Cout], Ho = (H + 2 pad - KH) / stride + 1 -> (out, mag):
      out[b][y][x][co] = sum_{ky,kx,ci} in[b][y s + ky - pad][x s + kx - pad][ci] w[co][ci][ky][kx]
    with zeros outside the image, then the epilogue of `gemm`."""
    B, H, W_, Cin = x.shape
    Cout, _, KH, KW = w.shape
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W_ + 2 * pad - KW) // stride + 1
    x64, w64 = x.double(), w.double()
    out = torch.zeros(B, Ho, Wo, Cout, dtype=torch.float64)
    mag = torch.zeros(B, Ho, Wo, Cout, dtype=torch.float64)
    for oy in range(Ho):
        for ox in range(Wo):
            for ky in range(KH):
                iy = oy * stride + ky - pad
                if iy < 0 or iy >= H:
                    continue
                for kx in range(KW):
                    ix = ox * stride + kx - pad
                    if ix < 0 or ix >= W_:
                        continue
                    px, wt = x64[:, iy, ix, :], w64[:, :, ky, kx]          # [B][Cin], [Cout][Cin]
                    out[:, oy, ox, :] += (px[:, None, :] * wt[None]).sum(-1)
                    mag[:, oy, ox, :] += (px[:, None, :].abs() * wt[None].abs()).sum(-1)
    return _epilogue(out, mag, bias, res, relu, relu_after)


def stem(img, w, bias):
    """pn_stem7x7s2_f32: img [B][3][H][W] (planar), w [64][3][7][7], stride 2, pad 3, + bias, ReLU
    -> channel-last (out [B][Ho][Wo][64], mag)."""
    return conv2d(img.permute(0, 2, 3, 1), w, bias, None, 2, 3, relu=True)


def maxpool3x3s2(x):
    """pn_maxpool3x3s2_nhwc_f32: 3x3, stride 2, pad 1 (the padding never wins: -inf) on
    x [B][H][W][C] -> [B][Ho][Wo][C], Ho = (H - 1) / 2 + 1.  Values are copied, so fp32 in,
    fp32 out, compared bit for bit."""
    B, H, W_, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W_ - 1) // 2 + 1
    out = torch.full((B, Ho, Wo, C), float("-inf"), dtype=x.dtype)
    for oy in range(Ho):
        for ox in range(Wo):
            for iy in range(max(2 * oy - 1, 0), min(2 * oy + 2, H)):
                for ix in range(max(2 * ox - 1, 0), min(2 * ox + 2, W_)):
                    out[:, oy, ox] = torch.maximum(out[:, oy, ox], x[:, iy, ix])
    return out


def mlearner_first(x, w1, b1):
    """First Matrix Learner layer: x [B][S][S], w1 [64][49] (tap = ky 7 + kx), 7x7, pad 3, + b1,
    ReLU -> (out [B][S S][64], mag)."""
    B, S, _ = x.shape
    out, mag = conv2d(x[..., None], w1.reshape(64, 1, 7, 7), b1, None, 1, 3, relu=True)
    return out.reshape(B, S * S, 64), mag.reshape(B, S * S, 64)


def mlearner_last(x, w3, b3):
    """Last Matrix Learner layer: x [B][S][S][64], w3 [49][64] (tap-major), 7x7, pad 3, + b3 ->
    (out [B][S][S], mag)."""
    out, mag = conv2d(x, w3.t().reshape(1, 64, 7, 7), b3, None, 1, 3)
    return out[..., 0], mag[..., 0]


# ------------------------------------------------------------------------------ Winograd
# F(2x2, 3x3) and F(4x4, 3x3) (Lavin & Gray): Y = A^T ((G g G^T) . (B^T d B)) A on (m + 2)^2
# patches d whose origin is (m ty - 1, m tx - 1), zeros outside the image, tiles that stick out
# clipped.
BT = {2: torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
                      dtype=torch.float64),
      4: torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
                       [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
                      dtype=torch.float64)}
G = {2: torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64),
     4: torch.tensor([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]],
                     dtype=torch.float64) / 24.0}
AT = {2: torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64),
      4: torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0],
                       [0, 1, -1, 8, -8, 1]], dtype=torch.float64)}


def wino_tiles(B, H, W_, m):
    return (H + m - 1) // m, (W_ + m - 1) // m


def wino_patches(x, m):
    """x [B][H][W][C] -> d [T][m + 2][m + 2][C] (float64), tile = (b th + ty) tw + tx."""
    B, H, W_, C = x.shape
    th, tw = wino_tiles(B, H, W_, m)
    pad = torch.zeros(B, m * th + 2, m * tw + 2, C, dtype=torch.float64)
    pad[:, 1:H + 1, 1:W_ + 1] = x.double()
    d = torch.stack([pad[:, m * ty:m * ty + m + 2, m * tx:m * tx + m + 2]
                     for ty in range(th) for tx in range(tw)], 1)          # [B][th tw][..]
    return d.reshape(B * th * tw, m + 2, m + 2, C)


def wino_input(x, m, absolute=False):
    """pn_winograd_f{23,43}_input_f32: V [(m + 2)^2][T][C] = B^T d B, position = i (m + 2) + j
    (absolute: |B|^T |d| |B|)."""
    d, bt = wino_patches(x, m), BT[m]
    if absolute:
        d, bt = d.abs(), bt.abs()
    V = torch.einsum("ik,tklc,jl->ijtc", bt, d, bt)
    return V.reshape((m + 2) ** 2, d.shape[0], d.shape[3])


def wino_weights(w, m, round_u=True, absolute=False):
    """pn_winograd_weights_f32: U [(m + 2)^2][Cout][Cin] = G g G^T in double, rounded to fp32 once
    (round_u; absolute: |that|)."""
    g, Gm = w.double(), G[m]
    # the kernel's order: t = G g, then U = t G^T, each entry three products summed left to right,
    # every product and sum rounded to double (no fused multiply-add)
    t = sum(Gm[:, k, None, None, None] * g[None, :, :, k, :] for k in range(3))      # [i][o][c][l]
    U = sum(t[:, None, :, :, k] * Gm[None, :, k, None, None] for k in range(3))     # [i][j][o][c]
    U = U.reshape((m + 2) ** 2, w.shape[0], w.shape[1])
    if round_u:
        U = U.float().double()
    return U.abs() if absolute else U


def wino_output(Mx, bias, B, H, W_, m, relu=False, absolute=False):
    """pn_winograd_f{23,43}_output_f32: Mx [(m + 2)^2][T][C] -> out [B][H][W][C] =
    act(A^T M A + bias), the tiles' overhang clipped (absolute: |A|^T M |A| + |bias|)."""
    th, tw = wino_tiles(B, H, W_, m)
    P, T, C = Mx.shape
    at = AT[m].abs() if absolute else AT[m]
    Y = torch.einsum("ik,kltc,jl->tijc", at, Mx.double().reshape(m + 2, m + 2, T, C), at)
    Y = Y.reshape(B, th, tw, m, m, C).permute(0, 1, 3, 2, 4, 5).reshape(B, th * m, tw * m, C)
    out = Y[:, :H, :W_]
    if bias is not None:
        out = out + (bias.double().abs() if absolute else bias.double())
    return out.clamp_min(0.0) if relu else out


def wino_gemm(V, U):
    """The (m + 2)^2 contractions M_p = V_p . U_p^T: [P][T][Cin] x [P][Cout][Cin] -> [P][T][Cout]."""
    return torch.einsum("ptc,poc->pto", V, U)


def wino_conv(x, w, bias, m, relu=False, round_u=True):
    """The whole Winograd form of the 3x3 pad-1 convolution -> (out [B][H][W][Cout], mag,
    stages): mag = |A|^T ((|B|^T |d| |B|) . |U|) |A| + |bias|, the quantity the algorithm's
    roundings scale with; stages = the largest |B|^T|d||B|, (..).|U| and mag (the exactness
    conditions of the integer cases)."""
    B, H, W_, _ = x.shape
    out = wino_output(wino_gemm(wino_input(x, m), wino_weights(w, m, round_u)), bias, B, H, W_, m,
                      relu)
    Va, Ua = wino_input(x, m, True), wino_weights(w, m, round_u, True)
    Ma = wino_gemm(Va, Ua)
    mag = wino_output(Ma, bias, B, H, W_, m, False, True)
    return out, mag, (float(Va.max()), float(Ma.max()), float(mag.max()))
