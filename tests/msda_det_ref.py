"""Host-side reference for the deterministic deformable-attention backward
(`pn_msda_bwd_det_f32`, csrc/msda_grad.hip): the definition of its grad_value restated in numpy,
and an input on which ONLY the order of the additions decides the fp32 result.  No GPU."""
import numpy as np
import torch

ORDER_SHAPES = [(4, 8), (2, 4)]          # (h, w), powers of two: every coordinate is exact in fp32
ORDER_NQ = 40
MIN_PLANTED = 8        # non-zero contributions of EACH id parity that make a destination "planted"


def scratch_lower_bound(B, N, Nq, L):
    """What any implementation needs: 8-byte records for every possible tap, a counter and a
    cursor per destination."""
    return 8 * B * Nq * 8 * L * 16 + 8 * B * 8 * N


def contributions(shapes, loc, aw):
    """The definition's contribution lists: {(b, token, head): [(id, coef float32, q), ...]} in
    ascending id, from loc [B][Nq][8][L][4][2] and aw [B][Nq][8][L][4] (numpy float32), with
    mmcv's in-map tests (ms_deform_attn_col2im_bilinear) in float32 arithmetic."""
    f = np.float32
    B, Nq, H8, L, P, _ = loc.shape
    starts = np.concatenate([[0], np.cumsum([h * w for h, w in shapes])[:-1]])
    out = {}
    for b in range(B):
        for q in range(Nq):
            for l, (Hl, Wl) in enumerate(shapes):
                for p in range(P):
                    for head in range(H8):
                        x, y = loc[b, q, head, l, p]
                        h_im, w_im = f(f(y) * f(Hl)) - f(0.5), f(f(x) * f(Wl)) - f(0.5)
                        # (the kernel may fuse the multiply and the subtraction; on the inputs
                        # built here both are exact, so it cannot matter)
                        if not (h_im > -1 and w_im > -1 and h_im < Hl and w_im < Wl):
                            continue
                        y0, x0 = int(np.floor(h_im)), int(np.floor(w_im))
                        lh, lw = f(h_im - f(y0)), f(w_im - f(x0))
                        hh, hw = f(f(1) - lh), f(f(1) - lw)
                        taps = [(y0, x0, f(hh * hw)), (y0, x0 + 1, f(hh * lw)),
                                (y0 + 1, x0, f(lh * hw)), (y0 + 1, x0 + 1, f(lh * lw))]
                        for t, (yy, xx, wt) in enumerate(taps):
                            if 0 <= yy < Hl and 0 <= xx < Wl:
                                tok = int(starts[l]) + yy * Wl + xx
                                cid = ((q * L + l) * 4 + p) * 4 + t
                                out.setdefault((b, tok, head), []).append(
                                    (cid, f(wt * f(aw[b, q, head, l, p])), q))
    for v in out.values():
        v.sort(key=lambda r: r[0])
    return out


def ordered_sum(records, gout_b, head, order=None):
    """acc = fmaf(coef, g, acc) over `records` in the given order (default: as listed), per
    channel, in float32: the product is formed exactly (float64) and the sum rounded once."""
    acc = np.zeros(32, np.float32)
    for cid, coef, q in (records if order is None else [records[i] for i in order]):
        g = gout_b[q, head * 32:(head + 1) * 32].astype(np.float64)
        acc = (acc.astype(np.float64) + np.float64(coef) * g).astype(np.float32)
    return acc


def order_case(seed=0, nq=ORDER_NQ, xs=(0.5, 1.0, 1.5, 2.0), ys=(0.0, 0.5, 1.0)):
    """An operator-form input (B = 1, Nq = `nq`, levels (4, 8) and (2, 4)) whose products are all
    exact: locations at pixel centres and half-pixel positions (tap weights 1, 0.5, 0.25),
    attention weights from {1, 0.5, 0.25, 0}, grad_output +- 2^0 .. 2^24.  Many (q, l, p) aim at
    the same few pixels.  Returns a dict of torch tensors (value, ss, starts, loc, aw, gout), the
    contribution lists, `expected` [1][N][8][32] (sequential float32 sum in ascending id) and
    `planted`: the destinations with at least MIN_PLANTED non-zero contributions of each id parity.
    `xs` / `ys`: the pixel coordinates the locations are drawn from (few values: long lists)."""
    rng = np.random.RandomState(seed)
    shapes, Nq, L = ORDER_SHAPES, nq, len(ORDER_SHAPES)
    N = sum(h * w for h, w in shapes)
    px = rng.choice(list(xs), size=(1, Nq, 8, L, 4))
    py = rng.choice(list(ys), size=(1, Nq, 8, L, 4))
    loc = np.zeros((1, Nq, 8, L, 4, 2), np.float32)
    for l, (h, w) in enumerate(shapes):
        loc[..., l, :, 0] = ((px[..., l, :] + 0.5) / w).astype(np.float32)
        loc[..., l, :, 1] = ((py[..., l, :] + 0.5) / h).astype(np.float32)
    aw = rng.choice([1.0, 0.5, 0.25, 0.0], size=(1, Nq, 8, L, 4)).astype(np.float32)
    gout = (rng.choice([-1.0, 1.0], size=(1, Nq, 256)) *
            np.exp2(rng.randint(0, 25, size=(1, Nq, 256)))).astype(np.float32)
    value = rng.randn(1, N, 8, 32).astype(np.float32)
    con = contributions(shapes, loc, aw)
    expected = np.zeros((1, N, 8, 32), np.float32)
    planted = []
    for (b, tok, head), recs in sorted(con.items()):
        expected[b, tok, head] = ordered_sum(recs, gout[b], head)
        # (both parities: a left-column tap has an even id, a right-column tap an odd one, and an
        # "evens, then odds" order differs from the ascending one only where both meet)
        if min(sum(1 for r in recs if r[1] != 0 and r[0] % 2 == k) for k in (0, 1)) >= MIN_PLANTED:
            planted.append((b, tok, head))
    ss = torch.tensor(shapes, dtype=torch.int64)
    starts = torch.cat([ss.new_zeros(1), (ss[:, 0] * ss[:, 1]).cumsum(0)[:-1]])
    t = torch.from_numpy
    return dict(shapes=shapes, N=N, Nq=Nq, L=L, value=t(value), ss=ss, starts=starts, loc=t(loc),
                aw=t(aw), gout=t(gout), contributions=con, expected=t(expected), planted=planted)
