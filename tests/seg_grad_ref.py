"""Float64 statement of what `SegmenterHeadGrad` (pair-net_amd/seg_grad.py) differentiates: the
shared heads on the outputs of all L decoder layers (`forward_head`, pairnet_head.py:236-243 /
baseline.py:254-296),

    qn = LayerNorm(q);  cls = Linear(qn);  me = Linear(ReLU(Linear(ReLU(Linear(qn)))))
    mask[l, b, q, p] = sum_c me[l, b, q, c] MF[b, p, c]          (einsum("bqc,bchw->bqhw"))

and the linear functional the segmentation loss's gradients define on them,

    F = sum cls * g_cls + sum mask[rows] * g_mask                 (rows < 0: no term)

with its VJP by autograd, the two mask products on their own (with the float64 sums of absolute
products for the error bounds) and the compact rows' image table.  Plain torch; shares no code with
the package."""
import numpy as np
import torch
import torch.nn.functional as F

PN = "transformer_decoder.post_norm."
HEAD_PARAMS = ("cls_embed.weight", "cls_embed.bias", "mask_embed.0.weight", "mask_embed.0.bias",
               "mask_embed.2.weight", "mask_embed.2.bias", "mask_embed.4.weight", "mask_embed.4.bias",
               PN + "weight", PN + "bias")
U, FLT_MIN = 2.0 ** -24, float(np.finfo(np.float32).tiny)


def heads(q_all, MF, P):
    """q_all [L, B, Q, C], MF [B, HW, C], P {name: tensor} -> cls [L, B, Q, nc], mask [L, B, Q, HW],
    me [L, B, Q, C]."""
    C = q_all.shape[-1]
    qn = F.layer_norm(q_all, (C,), P[PN + "weight"], P[PN + "bias"], 1e-5)
    cls = F.linear(qn, P["cls_embed.weight"], P["cls_embed.bias"])
    h = F.relu(F.linear(qn, P["mask_embed.0.weight"], P["mask_embed.0.bias"]))
    h = F.relu(F.linear(h, P["mask_embed.2.weight"], P["mask_embed.2.bias"]))
    me = F.linear(h, P["mask_embed.4.weight"], P["mask_embed.4.bias"])
    mask = torch.einsum("lbqc,bpc->lbqp", me, MF)
    return cls, mask, me


def functional(cls, mask, g_cls, g_mask, rows):
    """sum cls * g_cls + sum over the compact rows m with rows[m] >= 0 of mask[rows[m]] . g_mask[m]."""
    rows = torch.as_tensor(rows).long()
    ok = rows >= 0
    flat = mask.reshape(-1, mask.shape[-1])
    return (cls * g_cls).sum() + (flat[rows[ok]] * g_mask.reshape(len(rows), -1)[ok]).sum()


def vjp(q_all, MF, P, g_cls, g_mask, rows):
    """Autograd of the functional -> dict(q=, MF=, <parameter names>) in float64."""
    q = q_all.detach().double().requires_grad_()
    mf = MF.detach().double().requires_grad_()
    Pd = {k: v.detach().double().requires_grad_() for k, v in P.items() if k in HEAD_PARAMS}
    cls, mask, _ = heads(q, mf, Pd)
    functional(cls, mask, g_cls.double(), g_mask.double(), rows).backward()
    out = dict(q=q.grad, MF=mf.grad)
    out.update({k: v.grad for k, v in Pd.items()})
    return out


def row_images(L, counts):
    """Image of every compact row m = l * Ml + m_off[b] + j (layer-major, then image, n_b rows each;
    seg_losses.py) -> int array [L * Ml]."""
    per_layer = np.repeat(np.arange(len(counts)), counts)
    return np.tile(per_layer, L)


def products64(G, MF, me, rows, img):
    """The two mask products in float64 and the sums of absolute products:
    dme[m] = G[m] MF[img[m]] (0 for rows[m] < 0), dMF[b] = sum_{m in b, rows[m] >= 0} G[m]^T me[rows[m]].
    G [M, P], MF [B, P, C], me [N, C].  A failed row's G is not looked at (it may hold NaN)."""
    G, MF, me = G.double(), MF.double(), me.double()
    M, B, C = G.shape[0], MF.shape[0], MF.shape[2]
    dme, dme_mag = torch.zeros(M, C, dtype=torch.float64), torch.zeros(M, C, dtype=torch.float64)
    dMF, dMF_mag = torch.zeros_like(MF), torch.zeros_like(MF)
    for m in range(M):
        r, b = int(rows[m]), int(img[m])
        if r < 0:
            continue
        dme[m] = G[m] @ MF[b]
        dme_mag[m] = G[m].abs() @ MF[b].abs()
        dMF[b] += torch.outer(G[m], me[r])
        dMF_mag[b] += torch.outer(G[m].abs(), me[r].abs())
    return dme, dme_mag, dMF, dMF_mag


# ---- the kernel shapes of tests/test_seg_grad_kernels_gpu.py: (L, counts, h, w, Q) ---------------
KERNEL_CASES = {
    "one-chunk": (1, [1], 5, 7, 4),            # fewer pixels than one k-chunk
    "odd": (3, [3, 1], 13, 19, 6),             # nothing is a multiple of a tile
    "empty-image": (2, [2, 0, 5], 16, 32, 7),  # an image without rows, in the middle
    "ragged-tiles": (9, [20, 33], 50, 84, 40),  # row tiles ragged, several runs per tile
    "all-queries": (2, [100], 8, 8, 100),      # n_b = Q
    "production-pixels": (1, [5], 200, 334, 8),  # split-K with a ragged last slice
}


def kernel_case(name, seed=0, integer=False):
    """Seeded inputs of one case: G [M, P], MF [B, P, 256], me [L * B * Q, 256], rows int64 [M]
    (distinct queries per layer and image), img [M]."""
    L, counts, h, w, Q = KERNEL_CASES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    B, P, Ml = len(counts), h * w, sum(counts)
    M = L * Ml
    if integer:
        draw = lambda *s: torch.randint(-3, 4, s, generator=g).float()
    else:
        draw = lambda *s: torch.randn(*s, generator=g)
    G, MF, me = draw(M, P), draw(B, P, 256), draw(L * B * Q, 256)
    rows = []
    for l in range(L):
        for b, n in enumerate(counts):
            rows.append(torch.randperm(Q, generator=g)[:n].sort()[0] + (l * B + b) * Q)
    rows = torch.cat(rows).long() if rows else torch.zeros(0, dtype=torch.long)
    return dict(L=L, counts=counts, B=B, P=P, Q=Q, M=M, G=G, MF=MF, me=me, rows=rows,
                img=row_images(L, counts))
