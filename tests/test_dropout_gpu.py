"""GPU: the relation decoder's FFN dropout -- the counter-based kernels (csrc/dropout.hip) bit for
bit against the numpy reference of their mask, the taped Relation Fusion decoder's gradients under
FIXED masks against the float64 oracle (whose twelve nn.Dropout modules are replaced, here, by the
same masks), and the training step with `dropout=True`.

Bounds are the project's existing ones: forward 1e-4 absolute, every gradient tensor within 1e-4 of
its largest entry (tests/test_grad_gpu.py).  Measured on the MI355X: dropped forward 1.81e-6, worst
gradient ratio 7.78e-7 (rel_query_embed.weight; 8e-7 without dropout); this file 7.3 s wall."""
import time

import numpy as np
import pytest
import torch

import dropout_ref as ref
from helpers import golden, head_cfg, oracle_head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4

COUNTERS = [(0, 0, 0, 0), (0, 0, 0, 1), (0, 1, 0, 0), (0x0123456789abcdef, 0, 7, 11),
            (0xfedcba9876543210, 3, 0xffffffff, 5)]


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print("\ntests/test_dropout_gpu.py: %.1f s wall" % (time.time() - t0))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_keep_bits_equal_the_numpy_reference_bit_for_bit():
    from pairnet_amd import hip
    for n in (1, 3, 4, 5, 1023, 25600, 204800):
        for p in (0.1, 0.5, 0.999):
            for seed, subseq, step, site in COUNTERS:
                got = hip.dropout_keep(n, p, seed, subseq, step, site).cpu().numpy()
                want = ref.keep_mask(n, p, seed, subseq, step, site)
                assert got.dtype == np.uint8 and np.array_equal(got, want), \
                    (n, p, seed, subseq, step, site)
    # the pinned counts of tests/test_dropout.py, from the device
    for p, n, (seed, subseq, step, site), dropped in (
            (0.1, 204800, COUNTERS[0], 20304), (0.1, 25600, COUNTERS[1], 2542),
            (0.1, 204800, COUNTERS[2], 20409), (0.1, 204800, COUNTERS[3], 20543),
            (0.5, 204800, COUNTERS[0], 102164)):
        keep = hip.dropout_keep(n, p, seed, subseq, step, site)
        assert n - int(keep.sum()) == dropped
    assert float(hip.dropout_keep(4096, 0.0, 1, 2, 3, 4).float().min()) == 1.0


def test_dropout_values_in_place_out_of_place_and_with_a_residual():
    from pairnet_amd import hip
    g = torch.Generator().manual_seed(3)
    for n in (1, 3, 4, 5, 1023, 25600):
        x = torch.randn(n, generator=g)
        r = torch.randn(n, generator=g)
        xd, rd = x.to(DEV), r.to(DEV)
        xn, rn = x.numpy(), r.numpy()
        for p in (0.1, 0.5, 0.999):
            s = ref.scale(p)
            for seed, subseq, step, site in COUNTERS[2:4]:
                keep = ref.keep_mask(n, p, seed, subseq, step, site).astype(bool)
                want = np.where(keep, xn * s, np.float32(0.0)).astype(np.float32)   # one fp32 product
                out = torch.full((n + 4,), 7.0, device=DEV)        # (+ a guard behind the tail)
                hip.dropout(xd, out[:n], p, seed, subseq, step, site)
                assert np.array_equal(_bits(out[:n].cpu().numpy()), _bits(want)), (n, p)
                assert float(out[n:].min()) == 7.0 and float(out[n:].max()) == 7.0
                inpl = xd.clone()
                hip.dropout(inpl, inpl, p, seed, subseq, step, site)
                assert np.array_equal(_bits(inpl.cpu().numpy()), _bits(want)), (n, p)
                # residual: within 1 ulp of res + x s in float64 rounded once; exactly res if dropped
                want64 = (rn.astype(np.float64) + xn.astype(np.float64) * float(s)).astype(np.float32)
                buf = xd.clone()
                for src, dst in ((xd, torch.empty(n, device=DEV)), (buf, buf)):
                    hip.dropout(src, dst, p, seed, subseq, step, site, res=rd)
                    got = dst.cpu().numpy()
                    assert np.array_equal(_bits(got[~keep]), _bits(rn[~keep])), (n, p)
                    err = np.abs(got[keep].astype(np.float64) - want64[keep].astype(np.float64))
                    assert np.all(err <= np.spacing(np.abs(want64[keep]))), (n, p, err.max())
        # p = 0: bitwise x, bitwise x + res
        out = torch.empty(n, device=DEV)
        hip.dropout(xd, out, 0.0, 9, 0, 0, 0)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(xn))
        hip.dropout(xd, out, 0.0, 9, 0, 0, 0, res=rd)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(xn + rn))


def test_bad_arguments_are_refused_without_launching():
    from pairnet_amd import hip
    lib = hip.lib()
    x = torch.randn(64, device=DEV)
    y = torch.full((64,), 5.0, device=DEV)
    k = torch.full((64,), 9, device=DEV, dtype=torch.uint8)
    px, py, pk = x.data_ptr(), y.data_ptr(), k.data_ptr()
    a = (0, 0, 0, 0, None)                                     # seed, subseq, step, site, stream
    assert lib.pn_dropout_f32(None, None, py, 16, 0.1, *a) == -1
    assert lib.pn_dropout_f32(px, None, None, 16, 0.1, *a) == -1
    assert lib.pn_dropout_f32(px, None, py, 0, 0.1, *a) == -1
    assert lib.pn_dropout_f32(px, None, py, -4, 0.1, *a) == -1
    assert lib.pn_dropout_f32(px, None, py, (1 << 34) + 1, 0.1, *a) == -1
    for p in (1.0, -0.5, 2.0):
        assert lib.pn_dropout_f32(px, None, py, 16, p, *a) == -1
        assert lib.pn_dropout_keep_u8(pk, 16, p, *a) == -1
    assert lib.pn_dropout_f32(px + 4, None, py, 16, 0.1, *a) == -1
    assert lib.pn_dropout_f32(px, px + 8, py, 16, 0.1, *a) == -1
    assert lib.pn_dropout_f32(px, None, py + 4, 16, 0.1, *a) == -1
    assert lib.pn_dropout_keep_u8(None, 16, 0.1, *a) == -1
    assert lib.pn_dropout_keep_u8(pk, 0, 0.1, *a) == -1
    assert lib.pn_dropout_keep_u8(pk, (1 << 34) + 1, 0.1, *a) == -1
    torch.cuda.synchronize()
    assert float(y.min()) == 5.0 and float(y.max()) == 5.0 and int(k.min()) == 9 and int(k.max()) == 9


# ------------------------------------------------------------------ gradient parity, fixed masks
class _FixedDrop(torch.nn.Module):
    """Stands in for an nn.Dropout of the oracle: multiplies with keep / (1 - p) whatever the
    module's mode.  `mult`: float64, the oracle's sequence-first shape [R, B, C]."""

    def __init__(self, mult):
        super().__init__()
        self.mult = mult

    def forward(self, x):
        return x * self.mult


def _oracle64(sd):
    from oracle.head import OracleCrossHead2
    head = OracleCrossHead2(**head_cfg()).eval()
    head.load_state_dict({k: v.detach().cpu() for k, v in sd.items()}, strict=True)
    return head.double()


def test_relation_decoder_gradients_under_fixed_masks_equal_the_float64_oracle():
    """`reldec.npz`'s pair features through `relation_forward(pair, dropout=)` / `relation_backward`
    at p = 0.1 against autograd through the float64 oracle whose twelve nn.Dropout modules multiply
    with the SAME masks (`hip.dropout_keep` for the same counters, permuted from the tape's
    batch-major [B, R, C] to the oracle's [R, B, C]).  A wrong site or element-index mapping gives
    errors of the order of the gradients themselves, not of rounding."""
    from pairnet_amd import CrossHead2, RelationTailGrad
    from pairnet_amd.grad import FfnDropout
    from test_grad_gpu import _compare, _compare_params, _print, _rel_names
    fx = golden("reldec")
    _, sd, _ = oracle_head(int(fx["weight_seed"]))
    head = CrossHead2(**head_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    pair_seq = torch.from_numpy(fx["pair_feat"])                   # (2R, B, 256) seq-first
    B, R = pair_seq.shape[1], head.num_rel_query
    pair = pair_seq.transpose(0, 1).reshape(-1, 256).to(DEV)
    tape = RelationTailGrad(head)
    plain = tape.relation_forward(pair).clone()
    assert torch.equal(tape.relation_forward(pair, dropout=None), plain)
    assert torch.equal(tape.relation_forward(pair, dropout=FfnDropout(0.0, seed=1)), plain)
    assert float((plain.cpu() - torch.from_numpy(fx["rel_preds"])).abs().max()) < 1e-4
    drop = FfnDropout(0.1, seed=0x0123456789abcdef, subseq=1, step=7)
    rel = tape.relation_forward(pair, dropout=drop)
    assert tape.t["rel"] is rel
    assert torch.equal(tape.relation_forward(pair, dropout=drop), rel)       # a pure function
    assert float((rel - plain).abs().max()) > 1e-3                 # dropout was not ignored
    g = torch.randn(rel.shape, generator=torch.Generator().manual_seed(11))
    dpair, grads = tape.relation_backward(g)
    torch.cuda.synchronize()

    head_o = _oracle64(sd)
    s = float(ref.scale(drop.p))
    for i, layer in enumerate(head_o.relation_decoder.layers):
        d = drop._replace(layer=i)
        ffn = layer.ffns[0]
        assert isinstance(ffn.layers[0][2], torch.nn.Dropout) and isinstance(ffn.layers[2], torch.nn.Dropout)
        mult = []
        for which, C in ((0, head.rel_ffn), (1, 256)):
            keep = d.keep(B * R * C, which, device=DEV).cpu()
            assert np.array_equal(keep.numpy(), ref.keep_mask(B * R * C, d.p, d.seed, d.subseq,
                                                              d.step, 2 * i + which))
            mult.append(keep.view(B, R, C).permute(1, 0, 2).double() * s)
        ffn.layers[0][2] = _FixedDrop(mult[0])
        ffn.layers[2] = _FixedDrop(mult[1])
    pair_o = pair_seq.double().requires_grad_()
    r = head_o.rel_query_feat.weight.unsqueeze(1).repeat((1, B, 1))
    r_pos = head_o.rel_query_embed.weight.unsqueeze(1).repeat((1, B, 1))
    p_pos = head_o.rel_query_embed2.weight.unsqueeze(1).repeat((1, B, 1))
    for layer in head_o.relation_decoder.layers:          # (oracle/head.py relation_logits)
        r = layer(query=r, key=pair_o, value=pair_o, query_pos=r_pos, key_pos=p_pos,
                  query_key_padding_mask=None, key_padding_mask=None)
    rel_o = head_o.rel_cls_embed(r.transpose(0, 1))
    err = float((rel.cpu().double() - rel_o.detach()).abs().max())
    print("dropped forward: max |rel - rel_oracle| = %.2e" % err)
    assert err < 1e-4
    (rel_o * g.double()).sum().backward()
    report = []
    _compare("pair_feat", dpair.view(B, -1, 256).transpose(0, 1), pair_o.grad, report)
    _compare_params(grads, head_o, report, _rel_names())
    assert len(report) == 114
    _print(report)


# ------------------------------------------------------------------ the training step
def _batch():
    from test_losses_gpu import _outputs
    head, cls, masks, metas, gt_rels, gt_labels, gt_masks, pts = _outputs(2, H=96, W=128, bs=2)
    g = torch.Generator().manual_seed(2)
    feats = [torch.randn(2, c, 96 // s, 128 // s, generator=g).to(DEV)
             for c, s in zip((256, 512, 1024, 2048), (4, 8, 16, 32))]
    return head, feats, (metas, gt_rels, gt_labels, gt_masks), pts


def _keeps(tr, step):
    d = tr.dropout_descriptor(step)._replace(layer=2)
    return d.keep(2 * 100 * 256, 1, device=DEV).cpu()


@pytest.mark.parametrize("scope", ["tail", "head"])
def test_training_step_with_the_relation_decoder_dropout(scope):
    """(a) `dropout=False` is the step without the keyword, bitwise.  (b) `dropout=True` picks the
    reference's 0.1 from the config; `loss_r_cls` is the loss of the tape's DROPPED relation logits
    and not of the inference kernels'; the three terms dropout cannot reach equal the deterministic
    step's bitwise; the relation decoder's gradient segment equals a stand-alone taped run with the
    same descriptor and the same d loss / d rel.  (c) masks are a function of (seed, rank, step).
    (d) inference stays deterministic and dropout-free, and `write_back()` round-trips."""
    from pairnet_amd import CrossHead2, RelationTailGrad, TailTrainer
    from test_grad_gpu import _rel_names
    kw = dict(lr=1e-3, train_decoder=scope == "head")
    # (a)
    flat = []
    for extra in ({}, dict(dropout=False)):
        head, feats, (metas, gt_rels, gt_labels, gt_masks), pts = _batch()
        tr = TailTrainer(head, **kw, **extra)
        assert tr.drop_p == 0.0 and tr.dropout_descriptor() is None
        off = tr.step(feats, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
        flat.append((tr.flat_p.clone(), tr.flat_grad.clone()))
    for p_, g_ in flat[1:]:
        assert torch.equal(p_, flat[0][0]) and torch.equal(g_, flat[0][1])
    off = {k: v.clone() for k, v in off.items()}
    # (b)
    head, feats, (metas, gt_rels, gt_labels, gt_masks), pts = _batch()
    tr = TailTrainer(head, seed=5, dropout=True, **kw)
    assert tr.drop_p == 0.1 == head.rel_ffn_drop and tr.subseq == 0 and tr.steps == 0
    desc = tr.dropout_descriptor()
    assert (desc.p, desc.seed, desc.subseq, desc.step) == (0.1, 5, 0, 0)
    out = tr.step(feats, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
    torch.cuda.synchronize()
    assert tr.steps == 1
    for k in ("loss_match", "loss_sub_cls", "loss_obj_cls"):
        assert torch.equal(out[k], off[k]), k
    cls_d, mask_d = head._outputs(head._last_plan)                 # the step's own outputs
    dropped = tr.tape.t["rel"]
    assert float((dropped - cls_d["rel"]).abs().max()) > 1e-3
    lossmod = head._loss
    cum1 = lossmod.cum_samples.copy()
    up = {}
    lossmod.cum_samples = np.zeros_like(cum1)                      # (SeesawLoss accumulates)
    again = head.loss(dict(cls_d, rel=dropped), mask_d, gt_rels, None, gt_labels, gt_masks, metas,
                      point_coords=pts, grads=up)
    assert np.array_equal(lossmod.cum_samples, cum1)
    assert torch.equal(again["loss_r_cls"], out["loss_r_cls"])
    lossmod.cum_samples = np.zeros_like(cum1)
    inference = head.loss(cls_d, mask_d, gt_rels, None, gt_labels, gt_masks, metas, point_coords=pts)
    assert not torch.equal(inference["loss_r_cls"], out["loss_r_cls"])
    assert torch.equal(inference["loss_r_cls"], off["loss_r_cls"])
    print("loss_r_cls: dropped %.4f, inference %.4f" % (float(out["loss_r_cls"]),
                                                       float(inference["loss_r_cls"])))
    # stand-alone tape on an identically seeded, untrained head: same pair features, same
    # descriptor, same d loss / d rel -> the same relation-decoder gradients, bitwise
    g_step = {n: tr.tape.grads[n].clone() for n in _rel_names()}
    pair = tr.tape.t["pair"].clone()
    head0 = _batch()[0]
    alone = RelationTailGrad(head0)
    rel0 = alone.relation_forward(pair, dropout=desc)
    assert torch.equal(rel0, dropped)
    _, g0 = alone.relation_backward(up["rel"])
    for n in _rel_names():
        assert torch.equal(g0[n], g_step[n]), n
    grad1 = tr.flat_grad.clone()
    assert not torch.equal(grad1, flat[0][1])
    # (c)
    for _ in range(2):
        tr.step(feats, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
    assert not torch.equal(tr.flat_grad, grad1)
    head2, feats2 = _batch()[:2]
    twin = TailTrainer(head2, seed=5, dropout=True, **kw)
    for i in range(3):
        twin.step(feats2, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
        if i == 0:
            assert torch.equal(twin.flat_grad, grad1)
    assert torch.equal(twin.flat_p, tr.flat_p) and torch.equal(twin.flat_grad, tr.flat_grad)
    k0 = _keeps(tr, 0)
    assert not torch.equal(k0, _keeps(tr, 1)) and not torch.equal(_keeps(tr, 1), _keeps(tr, 2))
    assert torch.equal(k0, _keeps(twin, 0))
    for change in (dict(seed=6), dict(subseq=1)):
        # (the stand-alone tape's head was never stepped: it serves once more)
        head3, feats3 = (head0, feats) if "seed" in change else _batch()[:2]
        other = TailTrainer(head3, seed=change.get("seed", 5), dropout=True, **kw)
        other.subseq = change.get("subseq", 0)               # (the rank in a process group)
        assert not torch.equal(_keeps(other, 0), k0), change
        other.step(feats3, metas, gt_rels, gt_labels, gt_masks, point_coords=pts)
        assert not torch.equal(other.flat_grad, grad1), change
    # (d)
    outs, _ = head.forward(feats, metas)
    outs = {k: v.clone() for k, v in outs.items()}
    outs_b, _ = head.forward(feats, metas)
    for k in ("rel", "importance", "cls"):
        assert torch.equal(outs_b[k], outs[k]), k
    pl = head._last_plan
    taped = RelationTailGrad(head).forward(pl.q.clone(), pl.sub_pos, pl.obj_pos)
    torch.cuda.synchronize()
    for k in ("rel", "importance"):
        assert float((taped[k] - outs[k]).abs().max()) < 1e-4, k
    tr.write_back()
    fresh = CrossHead2(**head_cfg())
    fresh.load_state_dict(head.state_dict())
    fresh.to(DEV)
    outs_f, _ = fresh.forward(feats, metas)
    for k in ("rel", "importance", "cls"):
        assert torch.equal(outs_f[k], outs[k]), k


def test_detector_train_step_with_dropout_from_the_image():
    from pairnet_amd import build_detector, pairnet_r50
    det = build_detector(pairnet_r50())
    det.bbox_head.init_weights(seed=4)
    det.to(DEV)
    g = torch.Generator().manual_seed(9)
    H, W = 96, 128
    img = torch.randn(1, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4, batch_input_shape=(H, W))]
    gt_labels = [torch.tensor([3, 17, 90, 120])]
    gt_masks = [(torch.rand(4, H, W, generator=g) > 0.6).numpy()]
    gt_rels = [torch.tensor([[0, 1, 5], [2, 3, 17], [1, 0, 56]])]
    tr = det.trainer(dropout=True, seed=3)
    assert tr.drop_p == 0.1 and tr is det._trainer
    for _ in range(2):
        out = det.train_step(img, metas, gt_rels, None, gt_labels, gt_masks)
    assert tr.steps == 2
    assert set(out) == {"loss_r_cls", "loss_sub_cls", "loss_obj_cls", "loss_match", "grad_norm"}
    assert all(np.isfinite(float(v)) for v in out.values()) and float(out["grad_norm"]) > 0
    assert len(det.simple_test(img, metas)) == 1
