"""GPU: the two kernels of csrc/seg_grad.hip alone, against the float64 products of
tests/seg_grad_ref.py.

Bound form (tests/test_seg_loss_gpu.py, tests/test_baseline_loss_gpu.py):
|gpu - ref64| <= (c + a) * 2^-24 * mag + FLT_MIN per element; `mag` the float64 sum of absolute
products, a = max(4, 2 x the ratio torch's own fp32 matmul reaches on the same case), and c counted
from the kernels' summation order (labnotes R18.2; an fp32 MFMA is a k-ordered fmaf chain, one
rounding per step):

  pn_mask_embed_grad_f32     c = min(P, 2048) + ceil(P / 2048) - 1   one chain per 2048-pixel slice,
                                                                     then the slices added in order
  pn_mask_feature_grad_f32   c = L * max n_b                         one chain over the image's rows
"""
import numpy as np
import pytest
import torch

import seg_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U, FLT_MIN = R.U, R.FLT_MIN
_REF = {}


def _dev(t):
    return t.to(DEV).contiguous()


def _table(lists, B):
    """[img_off | order | tiles] from explicit per-image row lists (the layout of
    `hip.mask_grad_table`, for row sets it cannot describe)."""
    img_off, order, tiles = [0], [], []
    for b in range(B):
        s0 = len(order)
        order += lists[b]
        tiles += [v for s in range(s0, len(order), 32) for v in (b, s)]
        img_off.append(len(order))
    return torch.tensor(img_off + order + tiles, dtype=torch.int32), len(tiles) // 2


def _run(G, MF, me, rows, table, T, fill=float("nan")):
    """Both kernels on device inputs; the outputs are pre-filled with NaN: the kernels clear nothing
    themselves and must write everything."""
    from pairnet_amd import hip
    M, P = G.shape
    B = MF.shape[0]
    dme = torch.full((M, 256), fill, device=DEV)
    dMF = torch.full((B, P, 256), fill, device=DEV)
    scratch = torch.full((max(hip.mask_embed_grad_scratch_floats(T, P), 1),), fill, device=DEV)
    table = _dev(table)
    hip.mask_embed_grad(G, MF, rows, table, T, dme, scratch)
    hip.mask_feature_grad(G, me, rows, table, T, dMF)
    return dme, dMF


def _case(name, integer=False):
    key = (name, integer)
    if key not in _REF:               # the float64 reference is computed once per case
        c = R.kernel_case(name, integer=integer)
        c["ref"] = R.products64(c["G"], c["MF"], c["me"], c["rows"], c["img"])
        _REF[key] = c
    return _REF[key]


def _launch(c, **over):
    from pairnet_amd import hip
    table, T = hip.mask_grad_table(c["L"], c["counts"])
    d = dict(c, **over)
    return _run(_dev(d["G"]), _dev(d["MF"]), _dev(d["me"]), _dev(d["rows"]), table, T)


def _ratio(name, got, ref, mag, c):
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    ratio = float((err / (U * mag + FLT_MIN)).max()) if err.numel() else 0.0
    print("%s: worst ratio %.3f (bound %.1f)" % (name, ratio, c))
    assert not bool((err > c * U * mag + FLT_MIN).any()), (name, ratio, c)
    return ratio


def _allow(v32, v64, mag):
    r = (v32.double() - v64).abs() / (U * mag + FLT_MIN)
    return max(4.0, 2.0 * float(r.max())) if r.numel() else 4.0


@pytest.mark.parametrize("name", sorted(R.KERNEL_CASES))
def test_products_against_float64(name):
    from pairnet_amd import hip
    c = _case(name)
    dme64, dme_mag, dMF64, dMF_mag = c["ref"]
    dme, dMF = _launch(c)
    torch.cuda.synchronize()
    # torch's own fp32 matmuls on the same case (index_select / transpose / matmul on the device)
    G, MF, me, rows = _dev(c["G"]), _dev(c["MF"]), _dev(c["me"]), _dev(c["rows"])
    img = torch.from_numpy(c["img"]).to(DEV)
    t_dme = torch.zeros(c["M"], 256, device=DEV)
    t_dMF = torch.zeros(c["B"], c["P"], 256, device=DEV)
    for b in range(c["B"]):
        sel = torch.nonzero(img == b).view(-1)
        if sel.numel():
            Gb = G.index_select(0, sel)
            t_dme[sel] = Gb @ MF[b]
            t_dMF[b] = Gb.t() @ me.index_select(0, rows.index_select(0, sel))
    P, ks = c["P"], hip.MASK_GRAD_KSLICE
    assert ks == hip.lib().pn_mask_grad_kslice() == 2048
    c1 = min(P, ks) + (P + ks - 1) // ks - 1
    c2 = c["L"] * max(c["counts"])
    _ratio(name + " dme", dme, dme64, dme_mag, c1 + _allow(t_dme.cpu(), dme64, dme_mag))
    _ratio(name + " dMF", dMF, dMF64, dMF_mag, c2 + _allow(t_dMF.cpu(), dMF64, dMF_mag))
    print("%s torch fp32: dme ratio %.3f, dMF ratio %.3f" % (
        name, (_allow(t_dme.cpu(), dme64, dme_mag)) / 2, (_allow(t_dMF.cpu(), dMF64, dMF_mag)) / 2))


@pytest.mark.parametrize("name", sorted(R.KERNEL_CASES))
def test_small_integer_inputs_are_exact(name):
    """Entries in -3 .. 3: every partial sum is an integer below 2^24, so any index error shows and
    nothing else does."""
    c = _case(name, integer=True)
    dme64, _, dMF64, _ = c["ref"]
    assert float(dme64.abs().max()) < 2 ** 24 and float(dMF64.abs().max()) < 2 ** 24
    dme, dMF = _launch(c)
    assert torch.equal(dme.cpu().double(), dme64)
    assert torch.equal(dMF.cpu().double(), dMF64)


def test_two_calls_and_a_side_stream_give_the_same_bits():
    c = _case("ragged-tiles")
    dme, dMF = _launch(c)
    dme2, dMF2 = _launch(c)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        dme3, dMF3 = _launch(c)
    side.synchronize()
    torch.cuda.synchronize()
    for a, b in ((dme2, dMF2), (dme3, dMF3)):
        assert torch.equal(a, dme) and torch.equal(b, dMF)


@pytest.mark.parametrize("garbage", ["nan", "finite"])
@pytest.mark.parametrize("name,layer,image", [("odd", 1, 0), ("ragged-tiles", 4, 1)])
def test_failed_rows_contribute_nothing(name, layer, image, garbage):
    """One image's rows of one layer carry mask_rows = -1 and garbage in G: finite outputs, exact
    zero dme rows, and every other element bitwise what it is with those rows simply absent."""
    c = _case(name)
    L, counts, B = c["L"], c["counts"], c["B"]
    Ml = sum(counts)
    m0 = layer * Ml + sum(counts[:image])
    failed = list(range(m0, m0 + counts[image]))
    G, rows = c["G"].clone(), c["rows"].clone()
    rows[failed] = -1
    G[failed] = float("nan") if garbage == "nan" else 1e30
    dme, dMF = _launch(c, G=G, rows=rows)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dme).all()) and bool(torch.isfinite(dMF).all())
    assert float(dme[failed].abs().max()) == 0.0
    # the same problem without those rows: compact rows renumbered, an explicit table
    keep = [m for m in range(c["M"]) if m not in set(failed)]
    new = {m: i for i, m in enumerate(keep)}
    lists = [[new[m] for m in keep if c["img"][m] == b] for b in range(B)]
    table, T = _table(lists, B)
    dme_a, dMF_a = _run(_dev(c["G"][keep]), _dev(c["MF"]), _dev(c["me"]), _dev(c["rows"][keep]),
                        table, T)
    torch.cuda.synchronize()
    assert torch.equal(dme[keep], dme_a)
    assert torch.equal(dMF, dMF_a)
    # and within bound of the float64 products of the kept rows
    dme64, dme_mag, dMF64, dMF_mag = R.products64(c["G"], c["MF"], c["me"], rows, c["img"])
    assert float((dme.cpu().double() - dme64).abs().max()) <= 1e-3 * float(dme_mag.max())


def test_an_image_without_rows_gets_exact_zeros_without_clearing():
    c = _case("empty-image")
    dme, dMF = _launch(c)           # (outputs pre-filled with NaN)
    torch.cuda.synchronize()
    assert float(dMF[1].abs().max()) == 0.0 and bool(torch.isfinite(dMF).all())
    assert float(dMF[0].abs().max()) > 0 and float(dMF[2].abs().max()) > 0
    # no matched row in the whole batch
    from pairnet_amd import hip
    table, T = hip.mask_grad_table(3, [0, 0])
    assert T == 0
    dme0, dMF0 = _run(torch.empty(0, 35, device=DEV), _dev(torch.randn(2, 35, 256)),
                      _dev(torch.randn(12, 256)), torch.empty(0, dtype=torch.int64, device=DEV),
                      table, T)
    assert dme0.shape == (0, 256) and float(dMF0.abs().max()) == 0.0


def test_wrappers_refuse_bad_arguments():
    from pairnet_amd import hip
    c = _case("odd")
    table, T = hip.mask_grad_table(c["L"], c["counts"])
    table = _dev(table)
    G, MF, me, rows = _dev(c["G"]), _dev(c["MF"]), _dev(c["me"]), _dev(c["rows"])
    M, P, B = c["M"], c["P"], c["B"]
    dme, dMF = torch.empty(M, 256, device=DEV), torch.empty(B, P, 256, device=DEV)
    scr = torch.empty(hip.mask_embed_grad_scratch_floats(T, P), device=DEV)
    bad = [
        lambda: hip.mask_embed_grad(G.double(), MF, rows, table, T, dme, scr),           # dtype
        lambda: hip.mask_embed_grad(G, MF, rows.int(), table, T, dme, scr),
        lambda: hip.mask_embed_grad(G, MF, rows, table.long(), T, dme, scr),
        lambda: hip.mask_embed_grad(G.t().contiguous().t(), MF, rows, table, T, dme, scr),  # strides
        lambda: hip.mask_embed_grad(G, MF[:, :-1].contiguous(), rows, table, T, dme, scr),  # pixels
        lambda: hip.mask_embed_grad(G, MF, rows[:-1], table, T, dme, scr),
        lambda: hip.mask_embed_grad(G, MF, rows, table[:-1], T, dme, scr),
        lambda: hip.mask_embed_grad(G, MF, rows, table, T, dme[:-1], scr),
        lambda: hip.mask_embed_grad(G, MF, rows, table, T, dme, scr[:-1]),               # scratch
        lambda: hip.mask_embed_grad(G.cpu(), MF, rows, table, T, dme, scr),              # host
        lambda: hip.mask_feature_grad(G, me[:, :128].contiguous(), rows, table, T, dMF),
        lambda: hip.mask_feature_grad(G, me, rows, table, T, dMF[:, :-1].contiguous()),
        lambda: hip.mask_feature_grad(G, me.double(), rows, table, T, dMF),
        lambda: hip.mask_feature_grad(G, me, rows, table, T + 1, dMF),
        lambda: hip.mask_embed_grad(torch.empty(65536, 1, device=DEV), MF, rows, table, T, dme, scr),
    ]
    for i, f in enumerate(bad):
        with pytest.raises((ValueError, RuntimeError)):
            f()
            pytest.fail("call %d was accepted" % i)
