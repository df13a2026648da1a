"""CPU: the float64 statement behind `SegmenterHeadGrad` (tests/seg_grad_ref.py) pinned to the
reference-pinned oracle of the sibling head, its VJP against central differences, the flat gradient
layout against what autograd reaches, and the host-side run table of the mask-gradient kernels.
(The gradients' VALUES are GPU tests: tests/test_seg_grad_kernels_gpu.py, tests/test_seg_grad_gpu.py.)"""
import re
import os

import numpy as np
import pytest
import torch

import seg_grad_ref as R
from helpers import oracle_baseline_head
from oracle import seeded
from oracle.baseline_head import OracleCrossHeadBaseline


@pytest.fixture(scope="module")
def oracle_run():
    """One float64 run of the oracle's own `forward` (autograd on) on a seeded head at the smallest
    pyramid, with every decoder layer's output queries and the mask feature captured by hooks."""
    head_o, sd, _ = oracle_baseline_head(77)
    head_o = head_o.double()
    for p in head_o.parameters():
        p.requires_grad_(True)
    H, W = 64, 96
    feats = [f.double() for f in seeded.seeded_feats(78, 1, H, W)]
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)]
    seen = dict(q=[])
    hooks = [l.register_forward_hook(lambda m, i, o: seen["q"].append(o))
             for l in head_o.transformer_decoder.layers]
    hooks.append(head_o.pixel_decoder.register_forward_hook(
        lambda m, i, o: seen.__setitem__("mf", o[0])))
    cls, masks = OracleCrossHeadBaseline.forward.__wrapped__(head_o, feats, metas)
    for h in hooks:
        h.remove()
    return head_o, cls["cls"], masks["mask"], seen


def test_statement_reproduces_the_oracles_stacks(oracle_run):
    head_o, cls_o, mask_o, seen = oracle_run
    L, B, Q = cls_o.shape[:3]
    assert L == 9 and len(seen["q"]) == 9
    q_all = torch.stack([q.transpose(0, 1) for q in seen["q"]]).detach()     # [L, B, Q, 256]
    MF = seen["mf"].detach().flatten(2).transpose(1, 2)                      # [B, H2 W2, 256]
    P = {k: v.detach() for k, v in head_o.named_parameters()}
    cls, mask, _ = R.heads(q_all, MF, P)
    assert cls.dtype == torch.float64
    cls_o, mask_o = cls_o.detach(), mask_o.detach()
    e_cls = float((cls - cls_o.detach()).abs().max())
    e_mask = float((mask.view(mask_o.shape) - mask_o.detach()).abs().max())
    print("statement vs oracle: cls %.2e, mask %.2e" % (e_cls, e_mask))
    assert e_cls <= 1e-12 * max(1.0, float(cls_o.abs().max()))
    assert e_mask <= 1e-12 * max(1.0, float(mask_o.abs().max()))


def test_vjp_against_central_differences():
    """2 layers, 1 image, 3 queries, 4 x 5 pixels (8 channels, 5 class logits); one compact row is a
    failed one (-1)."""
    g = torch.Generator().manual_seed(5)
    L, B, Q, C, nc, P_ = 2, 1, 3, 8, 5, 20
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    P = {"cls_embed.weight": rn(nc, C), "cls_embed.bias": rn(nc), R.PN + "weight": rn(C) + 2.0,
         R.PN + "bias": rn(C)}
    for j in (0, 2, 4):
        P["mask_embed.%d.weight" % j], P["mask_embed.%d.bias" % j] = rn(C, C), rn(C)
    q, MF = rn(L, B, Q, C), rn(B, P_, C)
    rows = torch.tensor([0, 2, -1, 4])                   # rows into L * B * Q = 6
    g_cls, g_mask = rn(L, B, Q, nc), rn(4, 4, 5)
    got = R.vjp(q, MF, P, g_cls, g_mask, rows)
    inputs = dict(P, q=q, MF=MF)

    def value():
        cls, mask, _ = R.heads(inputs["q"], inputs["MF"], inputs)
        return float(R.functional(cls, mask, g_cls, g_mask, rows))

    eps, worst = 1e-6, 0.0
    for name, t in inputs.items():
        fd = torch.zeros_like(t)
        flat, fdf = t.view(-1), fd.view(-1)
        for i in range(flat.numel()):
            old = float(flat[i])
            flat[i] = old + eps
            up = value()
            flat[i] = old - eps
            dn = value()
            flat[i] = old
            fdf[i] = (up - dn) / (2 * eps)
        err = float((fd - got[name]).abs().max())
        scale = max(1.0, float(got[name].abs().max()))
        worst = max(worst, err / scale)
        assert err <= 1e-6 * scale, (name, err, scale)
    assert float(got["MF"].abs().max()) > 0 and float(got["q"].abs().max()) > 0
    print("central differences: worst relative error %.2e" % worst)


def test_layout_is_the_trunk_parameters_autograd_reaches(oracle_run):
    """`param_groups` names exactly the parameters the functional reaches behind the pixel decoder
    (decided by autograd through the oracle's own forward), each once; 64-aligned segments; monotone
    group ends."""
    from pairnet_amd import CrossHeadBaseline, CrossHead2, SegmenterHeadGrad
    from helpers import baseline_cfg, head_cfg
    head_o, cls_o, mask_o, _ = oracle_run
    g = torch.Generator().manual_seed(3)
    for p in head_o.parameters():
        p.grad = None
    ((cls_o * torch.randn(cls_o.shape, generator=g, dtype=torch.float64)).sum() +
     (mask_o * torch.randn(mask_o.shape, generator=g, dtype=torch.float64)).sum()).backward()
    reached = {n for n, p in head_o.named_parameters()
               if p.grad is not None and float(p.grad.abs().max()) > 0}
    trunk = {n for n in reached if not n.startswith("pixel_decoder.")}
    for head in (CrossHeadBaseline(**baseline_cfg()), CrossHead2(**head_cfg())):
        groups = SegmenterHeadGrad.param_groups(head)
        names = [n for _, ns in groups for n in ns]
        assert len(names) == len(set(names))
        assert set(names) == trunk, (sorted(set(names) - trunk)[:5], sorted(trunk - set(names))[:5])
        assert set(R.HEAD_PARAMS) <= set(names)
        off, ends = 0, []
        for _, ns in groups:
            for n in ns:
                assert off % 64 == 0
                off += (head._params[n].numel() + 63) // 64 * 64
            ends.append(off)
        assert ends == sorted(ends) and ends[-1] == SegmenterHeadGrad.size_of(head)
        assert [gname for gname, _ in groups][0] == "heads" and groups[-1][0] == "query"
    # nothing of the relation branch
    assert not any(n.startswith(("relation_decoder.", "rel_", "sub_query", "obj_query")) for n in names)


@pytest.mark.parametrize("L,counts", [(1, [1]), (3, [3, 1]), (2, [2, 0, 5]), (9, [20, 33]),
                                      (2, [100]), (4, [0, 0]), (3, [0, 40, 0, 7])])
def test_run_table_from_shapes_alone(L, counts):
    from pairnet_amd import hip
    tab, T = hip.mask_grad_table(L, counts)
    assert tab.dtype == torch.int32 and tab.dim() == 1
    tab = tab.numpy()
    B, Ml = len(counts), sum(counts)
    M = L * Ml
    assert tab.size == B + 1 + M + 2 * T
    img_off, order, tiles = tab[:B + 1], tab[B + 1:B + 1 + M], tab[B + 1 + M:].reshape(T, 2)
    img = R.row_images(L, counts)
    assert sorted(order.tolist()) == list(range(M))                 # every row once
    assert img_off[0] == 0 and img_off[-1] == M
    for b in range(B):
        part = order[img_off[b]:img_off[b + 1]]
        assert part.tolist() == np.nonzero(img == b)[0].tolist()    # the image's rows, layer-major
        assert len(part) == L * counts[b]
    # the tiles partition every image's part into runs of at most 32, none crossing an image
    covered = []
    for b, s in tiles.tolist():
        assert 0 <= b < B and img_off[b] <= s < img_off[b + 1] and (s - img_off[b]) % 32 == 0
        covered += list(range(s, min(s + 32, img_off[b + 1])))
    assert covered == list(range(M))
    assert T == sum((L * n + 31) // 32 for n in counts)


def test_run_table_refuses_what_the_kernels_cannot_index():
    from pairnet_amd import hip
    with pytest.raises(ValueError):
        hip.mask_grad_table(9, [4000, 4000])        # 72000 rows > 65535
    with pytest.raises(ValueError):
        hip.mask_grad_table(2, [3, -1])
    with pytest.raises(ValueError):
        hip.mask_grad_table(0, [3])


def test_abi_entries_are_declared_and_bound():
    from pairnet_amd import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "pairnet_hip.h")).read()
    for name in ("pn_mask_embed_grad_f32", "pn_mask_feature_grad_f32",
                 "pn_mask_embed_grad_scratch_floats", "pn_mask_grad_kslice"):
        assert name in hip.EXPORTS and re.search(r"\b%s\(" % name, header), name
    assert 'einsum("bqc,bchw->bqhw"' in header
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION
    from pairnet_amd import SegmenterHeadGrad, CrossHeadBaseline, api
    assert hasattr(CrossHeadBaseline, "seg_backward") and SegmenterHeadGrad.__name__ in api.__all__
