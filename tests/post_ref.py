"""float64 / integer statements of the kernels that DECIDE and of the box trunk's glue: the
label / probability kernels and the panoptic id maps of csrc/postproc.hip (up to
pn_pack_triplets_f32), the top-k entries of csrc/ppn.hip, all of csrc/detr.hip and
pn_sine_pe_valid_f32 (csrc/resize.hip), written from the formulas of the reference model
(pairnet_head.py:788-924, pairnet_bbox_head.py:193-359, :1056-1086, mmdet's Deformable-DETR
transformer and SinePositionalEncoding).  Value outputs come with `mag`, the computation on
absolute values, and `cond`, the count of fp32 roundings that an exp / log / sin / cos / pow
multiplies, per element and from the inputs alone; decision outputs are integers under a stated
tie rule (first index).  tests/test_post_refs.py pins every statement to torch and the oracle;
tests/test_post_kernels_gpu.py compares the kernels with them.  Inputs are fp32 CPU tensors; all
arithmetic is float64 (numpy or torch); nothing here comes from the kernels."""
import math

import numpy as np
import torch

INSTANCE_OFFSET = 1000
TWO_PI = 2.0 * math.pi


# ------------------------------------------------------------------------------ softmax family
def softmax(x, dim=-1):
    """p = exp(x - max) / sum exp(x - max) along `dim` -> (p, mag = p, cond).  The difference
    d = x - max is rounded once before the exponential, which turns it into a relative error
    |d| 2^-24 of that term: cond = |d_i| + sum_j p_j |d_j| (numerator and denominator)."""
    x64 = x.double()
    d = x64 - x64.amax(dim, keepdim=True)
    e = d.exp()
    p = e / e.sum(dim, keepdim=True)
    ad = torch.where(torch.isfinite(d), d.abs(), torch.zeros_like(d))     # exp(-inf) = 0 exactly
    return p, p, ad + (p * ad).sum(dim, keepdim=True)


def soft_nan_rows(x):
    """Rows whose softmax is NaN: a NaN entry, a +inf entry, or nothing but -inf."""
    return torch.isnan(x).any(-1) | (x == math.inf).any(-1) | (x == -math.inf).all(-1)


def argmax_first(v):
    """First index of the largest value along the last axis (numpy's argmax); NaN-free input."""
    a = np.asarray(v, dtype=np.float64)
    assert not np.isnan(a).any()
    return torch.from_numpy(np.argmax(a, axis=-1).astype(np.int64))


def cls_argmax(x, label_offset):
    """pn_cls_argmax_f32: label = offset + first argmax of softmax(x) over the columns but the
    last, score its probability -> (label, score, mag, cond, nan_rows).  A row whose softmax is
    NaN scores NaN; its label is offset + the first NaN among the admitted logits (torch.argmax of
    them), offset + 0 where there is none."""
    C = x.shape[-1]
    bad = soft_nan_rows(x)
    safe = torch.where(bad[:, None], torch.zeros_like(x), x)
    p, _, cond = softmax(safe)
    idx = argmax_first(p[:, :C - 1].numpy())
    score = p.gather(1, idx[:, None])[:, 0]
    cnd = cond.gather(1, idx[:, None])[:, 0]
    nan_adm = torch.isnan(x[:, :C - 1])
    first_nan = torch.where(nan_adm.any(-1), nan_adm.double().argmax(-1), torch.zeros_like(idx))
    idx = torch.where(bad, first_nan, idx)
    score = torch.where(bad, torch.full_like(score, math.nan), score)
    return idx + label_offset, score, score, cnd, bad


def rel_dists(x):
    """pn_rel_dists_f32: [0 | softmax(x)] -> (out, mag, cond), column 0 exactly +0."""
    p, mag, cond = softmax(x)
    z = torch.zeros(x.shape[0], 1, dtype=torch.float64)
    return torch.cat([z, p], 1), torch.cat([z, mag], 1), torch.cat([z, cond], 1)


def topk(v, k):
    """The k first of a stable sort on (-value in float64 with -0 = +0, index), per row ->
    int64 [B][k]."""
    a = np.asarray(v, dtype=np.float64) + 0.0
    assert not np.isnan(a).any()
    a = np.where(a == 0.0, 0.0, a)
    return torch.from_numpy(np.argsort(-a, axis=-1, kind="stable")[:, :k].astype(np.int64))


# ------------------------------------------------------------------------------ panoptic id maps
def panoptic(masks, labels, remap=None):
    """pn_panoptic_f32: per pixel the first argmax over the n planes, optionally mapped through
    `remap`; seg = id * 1000 + labels[id], area[id] += 1 -> (seg [HW], area [n])."""
    m = masks.double().numpy()
    bi = np.argmax(m, axis=0)
    if remap is not None:
        bi = np.asarray(remap)[bi]
    lab = np.asarray(labels)
    seg = bi.astype(np.int64) * INSTANCE_OFFSET + lab[bi]
    return torch.from_numpy(seg), torch.from_numpy(np.bincount(bi, minlength=m.shape[0]).astype(np.int32))


def panoptic_loop(up, labels, scores, last_real, max_rounds, seg0=None, want_ids=False):
    """pairnet_head.py:845-905 with the bookkeeping made explicit.  up [Q][HW] float64 (resized
    planes), labels int64 [Q], scores fp32 [Q].
      keep      queries with label != last_real (sic: the last REAL class) and score > 0.5, in order
      remap     kept position -> first kept position of the same label where label >= 80 (stuff)
      round     per pixel the first argmax over the alive kept planes; in the FIRST round
                duplicates are merged through remap; seg = rank * 1000 + label, rank = the
                position among the alive; segments of area <= 4 die; a round in which nothing
                died ends the loop (active = 0)
      rounds    number of rounds in which something died; all_gone: everything died
    At most `max_rounds` rounds are run.  nkeep = 0: seg is all ones.  Returns a dict with seg,
    nkeep, rounds, active, all_gone, kept, remap, alive, rank (rank[i] = alive positions before i)."""
    up = np.asarray(up, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    sc = np.asarray(scores, dtype=np.float32)
    HW = up.shape[1]
    kept = [q for q in range(len(lab)) if lab[q] != last_real and sc[q] > np.float32(0.5)]
    n = len(kept)
    klab = lab[kept] if n else np.zeros(0, np.int64)
    remap = np.arange(n)
    for i in range(n):
        if klab[i] >= 80:
            remap[i] = int(np.nonzero(klab[:i + 1] == klab[i])[0][0])
    alive = np.ones(n, dtype=bool)
    rank = np.arange(n)
    seg = None if seg0 is None else np.asarray(seg0).copy()
    ids = None
    active, rounds, all_gone, first = 1, 0, 0, True
    for _ in range(max_rounds):
        if not active:
            break
        if n == 0:
            seg = np.ones(HW, dtype=np.int64)
            active = 0
            continue
        pos = np.nonzero(alive)[0]
        bi = pos[np.argmax(up[np.asarray(kept)[pos]], axis=0)]
        if first:
            bi = remap[bi]
            first = False
        ids = bi
        seg = rank[bi].astype(np.int64) * INSTANCE_OFFSET + klab[bi]
        area = np.bincount(bi, minlength=n)
        small = alive & (area <= 4)
        if not small.any():
            active = 0
            continue
        alive = alive & ~small
        rank = np.cumsum(alive) - alive
        rounds += 1
        if not alive.any():
            all_gone, active = 1, 0
    out = dict(seg=seg, nkeep=n, rounds=rounds, active=active, all_gone=all_gone,
               kept=np.asarray(kept, dtype=np.int32), remap=remap.astype(np.int32),
               alive=alive.astype(np.int32), rank=rank.astype(np.int32), klab=klab)
    if want_ids:
        out["ids"] = ids
    return out


# ------------------------------------------------------------------------------ box trunk glue
def zero_rows(x, valid):
    """out = where(valid row, x, +0): a select, so NaN / inf in an invalid row give +0."""
    return torch.where(valid.bool()[..., None], x, torch.zeros_like(x))


def sigmoid(x):
    return 1.0 / (1.0 + (-x.double()).exp())


POS_ARG_L = 9       # s (4: exp 2, add, divide), 2 pi (constant, product), dim_t (pow 2), the quotient


def box_pos_embed(unact):
    """pn_box_pos_embed_f32: ref = sigmoid(unact) [rows][4]; emb[r][j*128 + i] = sin (i even) /
    cos (i odd) of ref[r][j] 2 pi / 10000^(2 (i // 2) / 128) -> (ref, emb, emb_mag = 1, emb_cond).
    emb_cond = POS_ARG_L |argument|: the roundings of the argument, which sin / cos pass on 1:1."""
    s = sigmoid(unact)
    i = torch.arange(128, dtype=torch.float64)
    dim_t = 10000.0 ** (2.0 * torch.div(i, 2, rounding_mode="floor") / 128.0)
    v = (s * TWO_PI)[:, :, None] / dim_t
    emb = torch.where((torch.arange(128) % 2 == 1)[None, None, :], v.cos(), v.sin())
    rows = unact.shape[0]
    return s, emb.reshape(rows, 512), torch.ones(rows, 512, dtype=torch.float64), \
        (POS_ARG_L * v.abs()).reshape(rows, 512)


def box_refine(delta, ref_in):
    """sigmoid(delta + log(max(x, 1e-5) / max(1 - x, 1e-5))), x = clamp(ref_in, 0, 1) ->
    (out, mag = out, cond).  z = delta + log q carries 3 roundings of q (1 - x, the fp32 constant
    1e-5f, the quotient), 2 |log q| of the logarithm and |z| of the sum; the sigmoid turns an
    absolute error of z into at most the same relative error of the output."""
    x = ref_in.double().clamp(0.0, 1.0)
    lq = (x.clamp_min(1e-5) / (1.0 - x).clamp_min(1e-5)).log()
    z = delta.double() + lq
    out = sigmoid(z)
    cond = torch.where(torch.isfinite(z), 3.0 + 2.0 * lq.abs() + z.abs(), torch.zeros_like(z))
    return out, out, cond


def box_sampling(offaw, ref, L, vr=None, rows_per_image=0):
    """mmcv MultiScaleDeformableAttention with 4-d reference points, 8 heads, 4 points:
    offaw row = [offsets 8 x L*4 x 2 | logits 8 x L*4]; weights = softmax over the L*4 logits of
    a head; location = ref.xy * r + offset / 4 * (ref.wh * r) * 0.5, r = the valid ratio (x, y) of
    the sampled level of the row's image (1 without) -> (loc, loc_mag, aw, aw_mag, aw_cond)."""
    rows, NP = offaw.shape[0], L * 4
    o = offaw.double()
    off = o[:, :8 * NP * 2].reshape(rows, 8, NP, 2)
    lg = offaw[:, 8 * NP * 2:8 * NP * 3].reshape(rows, 8, NP)
    aw, aw_mag, aw_cond = softmax(lg)
    r = torch.ones(rows, L, 2, dtype=torch.float64)
    if vr is not None:
        r = vr.double()[torch.arange(rows) // rows_per_image]
    r = r.repeat_interleave(4, 1)[:, None]                                 # [rows][1][NP][2]
    c = ref.double()[:, None, None, :2] * r
    h = off / 4.0 * (ref.double()[:, None, None, 2:] * r) * 0.5
    return c + h, c.abs() + h.abs(), aw, aw_mag, aw_cond


def token_sampling(offaw, vr, shapes):
    """Encoder self-attention operands on a padded batch (mmdet get_reference_points): the token
    n of level lq at (x, y) has ref = ((x + .5) / (vr[b][lq].x W_lq), (y + .5) / (vr[b][lq].y
    H_lq)); location at sampled level ls = ref * vr[b][ls] + offset / (W_ls, H_ls).
    offaw [B][N][...], vr [B][L][2] -> (loc, loc_mag, aw, aw_mag, aw_cond), [B][N][8][L*4](x2)."""
    B, N = offaw.shape[:2]
    L = len(shapes)
    NP = L * 4
    o = offaw.double()
    off = o[..., :8 * NP * 2].reshape(B, N, 8, NP, 2)
    aw, aw_mag, aw_cond = softmax(offaw[..., 8 * NP * 2:8 * NP * 3].reshape(B, N, 8, NP))
    v = vr.double()
    refs = []
    for lvl, (h, w) in enumerate(shapes):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64) + 0.5,
                                torch.arange(w, dtype=torch.float64) + 0.5, indexing="ij")
        rx = xs.reshape(-1)[None] / (v[:, None, lvl, 0] * w)
        ry = ys.reshape(-1)[None] / (v[:, None, lvl, 1] * h)
        refs.append(torch.stack((rx, ry), -1))
    ref = torch.cat(refs, 1)                                                # [B][N][2]
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
    c = ref[:, :, None, None, :] * v.repeat_interleave(4, 1)[:, None, None]
    d = off / wh.repeat_interleave(4, 0)
    return c + d, c.abs() + d.abs(), aw, aw_mag, aw_cond


def query_score(logits):
    """score[b][q] = max_c softmax over the QUERIES of logits[b][:, c] -> (score, mag = score,
    cond = the largest cond of a (q, c) term of that query: |max a - max b| <= max |a - b|)."""
    p, _, cond = softmax(logits, dim=1)
    return p.amax(-1), p.amax(-1), cond.amax(-1)


def box_triplets(s_cls, o_cls, s_box, o_box, img_h, img_w, sf, rescale):
    """pairnet_bbox_head.py:1056-1086 on [subjects | objects]: label = 1 + first argmax of the
    logits, score = its softmax probability; box cxcywh -> xyxy, scaled to the image, clamped into
    it, divided by the four scale factors (x1 / sf0, y1 / sf1, x2 / sf2, y2 / sf3) when rescaling
    -> (labels [2R], det [2R][5], mag, cond [2R])."""
    cls = torch.cat([s_cls, o_cls], 0)
    box = torch.cat([s_box, o_box], 0).double()
    labels = argmax_first(cls.double().numpy()) + 1
    p, _, _ = softmax(cls)
    d = cls.double() - cls.double().amax(-1, keepdim=True)
    ad = torch.where(torch.isfinite(d), d.abs(), torch.zeros_like(d))
    score = p.amax(-1)
    cond = (p * ad).sum(-1)                  # the numerator is exp(0) = 1: the denominator alone
    cx, cy, w, h = box.unbind(-1)
    div = [float(v) if rescale else 1.0 for v in sf]
    cols, mags = [], []
    for centre, half, size, dv in ((cx, -0.5 * w, img_w, div[0]), (cy, -0.5 * h, img_h, div[1]),
                                   (cx, 0.5 * w, img_w, div[2]), (cy, 0.5 * h, img_h, div[3])):
        cols.append(((centre + half) * size).clamp(0.0, float(size)) / dv)
        mags.append((centre.abs() + half.abs()) * size / abs(dv))
    det = torch.stack(cols + [score], -1)
    return labels, det, torch.stack(mags + [score], -1), cond


def sine_pe(h, w, C, vh, vw, temperature, offset, add=None):
    """mmdet SinePositionalEncoding(num_feats = C / 2, normalize=True, scale = 2 pi, eps = 1e-6)
    of the mask that is False on [0, vh) x [0, vw), token-major: out [h*w][C] = [pos_y | pos_x],
    sin (even) / cos (odd) of embed / T^(2 (i // 2) / num_feats), embed = (cumsum of the
    not-padded flags + offset) / (its last entry + eps) * 2 pi; `add` [C] is added.
    -> (out, mag = 1 + |add|, cond, wild): cond = |argument| (7 + ln T * exponent) -- the
    normaliser's sum, the quotient, 2 pi (constant and product), the power (2), the exponent's
    quotient (which the power multiplies by ln T * exponent), the last quotient; wild marks the
    elements whose normaliser is 0 and whose offset is not (argument ~ 3e6: no bound means
    anything)."""
    nf = C // 2
    nm = np.zeros((h, w), dtype=np.float64)
    nm[:vh, :vw] = 1.0
    ye, xe = nm.cumsum(0), nm.cumsum(1)
    ny, nx = ye[-1:, :], xe[:, -1:]
    ey = (ye + offset) / (ny + 1e-6) * TWO_PI
    ex = (xe + offset) / (nx + 1e-6) * TWO_PI
    i = np.arange(nf)
    expo = 2.0 * (i // 2) / nf
    dim_t = float(temperature) ** expo
    arg = np.concatenate([ey[:, :, None] / dim_t, ex[:, :, None] / dim_t], -1)       # [h][w][C]
    odd = np.concatenate([i % 2 == 1, i % 2 == 1])
    out = np.where(odd, np.cos(arg), np.sin(arg))
    cnt = 7.0 + math.log(float(temperature)) * np.concatenate([expo, expo])
    wild = np.concatenate([np.broadcast_to(((ny == 0) & (offset != 0))[:, :, None], (h, w, nf)),
                           np.broadcast_to(((nx == 0) & (offset != 0))[:, :, None], (h, w, nf))], -1)
    mag = np.ones((h, w, C))
    if add is not None:
        a = add.double().numpy()
        out, mag = out + a, mag + np.abs(a)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).reshape(h * w, C)
    return t(out), t(mag), t(np.abs(arg) * cnt), t(wild)


# ------------------------------------------------------------------------------ the value bound
U = 2.0 ** -24
FLT_MIN = 2.0 ** -126


def value_bound(ref, mag, L, cond, o32):
    """(L + a + cond) 2^-24 mag + FLT_MIN per element, a = max(4, 2 x the ratio torch's fp32
    evaluation `o32` of the same operation reaches against `ref`, net of cond) -> (bound, a).
    This is what the GPU file asserts of every value output; the admissibility of an index on
    random inputs uses it as the distance within which two scores cannot be told apart."""
    ref, mag = ref.double(), mag.double()
    cond = torch.zeros_like(mag) if cond is None else cond.double().expand_as(mag)
    err = ((o32.double() - ref).abs() - FLT_MIN - U * cond * mag).clamp_min(0.0)
    ratio = torch.where(err > 0, err / (U * mag), torch.zeros_like(err))
    ratio = ratio[torch.isfinite(ratio)]
    a = max(4.0, 2.0 * float(ratio.max())) if ratio.numel() else 4.0
    return (L + a + cond) * U * mag + FLT_MIN, a


SOFT_L = 14         # exp (2) on the numerator; exp (2), 3 in-lane adds, 6 shuffle adds on the
#                     denominator; the quotient
