"""float64 statements for the ResNeXt path: the grouped 3x3 convolution pn_conv2d_grouped_nhwc_f32
(csrc/grouped_conv.hip) and the ResNeXt backbone (mmdet's, restated from memory, unpinned:
configs/deformable_detr/pairnet_rnext101_vg.py:9-21), with the cases and the seeded state the tests
share.  No new arithmetic: the convolution is tests/mm_ref.conv2d on each group's channel slice;
the backbone is torch's own ops in float64.  tests/test_resnext_refs.py pins the first to
F.conv2d(groups=G); tests/test_grouped_conv_gpu.py compares the kernels with both."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

import mm_ref as R

# pixel tile of csrc/grouped_conv.hip: 16 output columns x 8 (stride 1) / 4 (stride 2) output rows,
# 64 channels per workgroup = 8 / 4 / 2 / 1 groups of 8 / 16 / 32 / 64 channels
TILE_W, TILE_H, WG_CHANNELS = 16, {1: 8, 2: 4}, 64

# (B, H, W, G, Cg, stride)
CASES = [
    # the issue's list
    (2, 7, 9, 32, 8, 1), (1, 9, 11, 32, 16, 2), (1, 6, 5, 32, 32, 1), (1, 5, 7, 32, 64, 2),
    (1, 1, 1, 1, 8, 1), (1, 2, 3, 3, 8, 2), (2, 8, 8, 5, 16, 2),
    # one more than the pixel tile on both sides, per Cg: stride 1 -> 9 x 17 outputs; stride 2 ->
    # 5 x 17 outputs from an even (10 x 34) and an odd (9 x 33) map
    (1, 9, 17, 3, 8, 1), (1, 9, 17, 2, 16, 1), (1, 9, 17, 1, 32, 1), (1, 9, 17, 1, 64, 1),
    (1, 10, 34, 3, 8, 2), (1, 9, 33, 2, 16, 2), (1, 10, 34, 1, 32, 2), (1, 9, 33, 1, 64, 2),
    # G no multiple of the groups a workgroup owns (8 / 4 / 2), more than one channel block
    (1, 4, 5, 11, 8, 1), (1, 5, 4, 6, 16, 2), (1, 3, 18, 3, 32, 1),
    # stride 2 at even H / W (the list above has it at odd ones)
    (1, 6, 8, 2, 64, 2),
]


def case_name(c):
    return "B%d %dx%d G%d Cg%d s%d" % c


def relu_of(ci):
    """ReLU on every other case; the stride-2 cases at even and odd sizes get both (they sit at
    indices of both parities)."""
    return ci % 2 == 0


def gen(seed):
    return torch.Generator().manual_seed(seed)


def exact_operands(c, seed):
    """Integers: x in [-8, 8], w in [-4, 4], a bias distinct per channel (a group mix-up moves it)
    -> (x [B][H][W][C], w [C][Cg][3][3], bias [C]).  9 Cg 32 + C <= 18432 + 2048 < 2^24."""
    B, H, W, G, Cg, s = c
    g = gen(seed)
    C = G * Cg
    x = torch.randint(-8, 9, (B, H, W, C), generator=g).float()
    w = torch.randint(-4, 5, (C, Cg, 3, 3), generator=g).float()
    bias = (torch.arange(C) - C // 2).float()
    return x, w, bias


def random_operands(c, seed):
    B, H, W, G, Cg, s = c
    g = gen(seed)
    C = G * Cg
    x = torch.randn(B, H, W, C, generator=g) * 2.0
    w = torch.randn(C, Cg, 3, 3, generator=g) * (9 * Cg) ** -0.5
    bias = torch.randn(C, generator=g) + 0.01 * torch.arange(C)
    return x, w, bias


def pack_weight(w):
    """torch's [G Cg][Cg][3][3] -> Wg [G][Cg][(ky 3 + kx) Cg + ci] (flat [G Cg][9 Cg])."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def chain(Cg):
    """Roundings per output of k_conv3x3_grouped, counted from its source: ONE accumulator chain
    over the taps and their channels in a fixed order -- 9 Cg products through
    v_mfma_f32_16x16x4_f32, nothing is merged (at Cg = 8 the other group's 72 products are exact
    zeros: no rounding) -- then the bias."""
    return 9 * Cg + 1


def grouped_conv(x, w, bias, G, stride, relu):
    """x [B][H][W][G Cg] fp32, w [G Cg][Cg][3][3], bias [G Cg] -> (value, mag) in float64: group g
    is mm_ref.conv2d (3x3, pad 1) on channels [g Cg, (g + 1) Cg)."""
    Cg = w.shape[1]
    assert x.shape[3] == G * Cg and w.shape[0] == G * Cg and tuple(w.shape[2:]) == (3, 3)
    outs, mags = [], []
    for g in range(G):
        sl = slice(g * Cg, (g + 1) * Cg)
        o, m = R.conv2d(x[..., sl], w[sl], bias[sl], None, stride, 1, relu=relu)
        outs.append(o)
        mags.append(m)
    return torch.cat(outs, -1), torch.cat(mags, -1)


# ------------------------------------------------------------------------------ the backbone
BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}


def width(planes, groups, base_width):
    return (planes * base_width // 64) * groups


def param_shapes(depth=101, groups=32, base_width=8):
    """mmdet's / torchvision's ResNeXt state dict: names -> shapes."""
    s = OrderedDict()

    def bn(prefix, c):
        for n in ("weight", "bias", "running_mean", "running_var"):
            s["%s.%s" % (prefix, n)] = (c,)
        s[prefix + ".num_batches_tracked"] = ()

    s["conv1.weight"] = (64, 3, 7, 7)
    bn("bn1", 64)
    cin = 64
    for i, (planes, blocks) in enumerate(zip((64, 128, 256, 512), BLOCKS[depth])):
        wd = width(planes, groups, base_width)
        for b in range(blocks):
            p = "layer%d.%d." % (i + 1, b)
            s[p + "conv1.weight"] = (wd, cin, 1, 1)
            bn(p + "bn1", wd)
            s[p + "conv2.weight"] = (wd, wd // groups, 3, 3)
            bn(p + "bn2", wd)
            s[p + "conv3.weight"] = (planes * 4, wd, 1, 1)
            bn(p + "bn3", planes * 4)
            if b == 0:
                s[p + "downsample.0.weight"] = (planes * 4, cin, 1, 1)
                bn(p + "downsample.1", planes * 4)
            cin = planes * 4
    return s


def seeded_state(seed, depth=101, groups=32, base_width=8):
    """He-seeded convolutions (std sqrt(2 / fan_in)); BatchNorm statistics away from the identity
    so that folding is exercised; each block's last norm has a small gamma (0.25 .. 0.5), which
    keeps the 33 residual additions from growing the maps by orders of magnitude."""
    g = gen(seed)
    out = OrderedDict()
    for k, shape in param_shapes(depth, groups, base_width).items():
        if k.endswith("num_batches_tracked"):
            out[k] = torch.zeros((), dtype=torch.int64)
        elif k.endswith("running_var"):
            out[k] = torch.rand(shape, generator=g) + 0.5
        elif k.endswith("running_mean"):
            out[k] = torch.randn(shape, generator=g) * 0.1
        elif len(shape) == 1 and k.endswith("weight"):
            out[k] = torch.rand(shape, generator=g) * 0.25 + 0.25 if ".bn3." in k \
                else torch.rand(shape, generator=g) + 0.5
        elif len(shape) == 1:
            out[k] = torch.rand(shape, generator=g) * 0.2 - 0.1
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            out[k] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
    return out


def resnext(P, img, groups=32, base_width=8, depth=101, dtype=torch.float64):
    """mmdet's ResNeXt forward (style "pytorch": the stride on conv2; eval-mode BatchNorm, eps
    1e-5; out_indices 0-3) on img [B][3][H][W] with the state dict P -> [C2, C3, C4, C5] (NCHW)."""
    P = {k: v.to(dtype) for k, v in P.items() if v.dim() > 0}

    def bn(x, p):
        return F.batch_norm(x, P[p + ".running_mean"], P[p + ".running_var"], P[p + ".weight"],
                            P[p + ".bias"], False, 0.0, 1e-5)

    x = F.relu(bn(F.conv2d(img.to(dtype), P["conv1.weight"], stride=2, padding=3), "bn1"))
    x = F.max_pool2d(x, 3, stride=2, padding=1)
    outs = []
    for i, blocks in enumerate(BLOCKS[depth]):
        for b in range(blocks):
            p = "layer%d.%d." % (i + 1, b)
            stride = 2 if (b == 0 and i > 0) else 1
            y = F.relu(bn(F.conv2d(x, P[p + "conv1.weight"]), p + "bn1"))
            y = F.relu(bn(F.conv2d(y, P[p + "conv2.weight"], stride=stride, padding=1,
                                   groups=groups), p + "bn2"))
            y = bn(F.conv2d(y, P[p + "conv3.weight"]), p + "bn3")
            if b == 0:
                x = bn(F.conv2d(x, P[p + "downsample.0.weight"], stride=stride),
                       p + "downsample.1")
            x = F.relu(y + x)
        outs.append(x)
    return outs
