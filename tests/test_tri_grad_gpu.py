"""GPU: `pn_triplet_heads_bwd_f32` (csrc/tri_grad.hip) alone against float64 under the bound of
tests/tri_grad_ref.py, and `PSGTr2HeadGrad` (pair-net_amd/seg_grad.py) -- the triplet-loss gradients
carried through `PSGTrHead2`'s heads and the nine masked decoder layers -- against float64 autograd:
the heads through the statement of tests/tri_grad_ref.py, the decoder through the reference-pinned
oracle's layers under the GPU's own attention-mask bits (as tests/test_seg_grad_gpu.py does for the
same layers).  Tolerance of the tape: 1e-4 of each tensor's largest entry; the taped forward
reproduces the inference forward's outputs to 1e-4 absolute.  A seeded `PSGTrHead2` at the 64 x 96
pyramid, two images with 3 and 1 matched rows."""
import pytest
import torch

import tri_grad_ref as R
from helpers import oracle_psgtr2_head, psgtr2_cfg
from oracle import seeded
from oracle.psgtr_head2 import OraclePSGTrHead2
from test_grad_gpu import _compare, _compare_params, _print, _unpack_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 64, 96
COUNTS = [3, 1]
_S = {}


# ------------------------------------------------------------------------------ the kernel alone
def _run_kernel(case):
    from pairnet_amd import hip
    d = lambda t: t.to(DEV).contiguous()
    N, C1, Cr1 = case["N"], case["C1"], case["Cr1"]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    out = dict(dqn=d(case["pre"]) if case["add"] else nan(N, 256), dWsub=nan(C1, 256),
               dbsub=nan(C1), dWobj=nan(C1, 256), dbobj=nan(C1), dWrel=nan(Cr1, 256), dbrel=nan(Cr1))
    hip.tri_heads_bwd(d(case["dsub"]), d(case["dobj"]), d(case["drel"]), d(case["qn"]),
                      d(case["Wsub"]), d(case["Wobj"]), d(case["Wrel"]), out["dqn"], out["dWsub"],
                      out["dbsub"], out["dWobj"], out["dbobj"], out["dWrel"], out["dbrel"],
                      add=case["add"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_alone_against_float64(name):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    case = R.kernel_case(name)
    got = _run_kernel(case)
    bad = []
    for key in R.OUTPUTS:
        ok, worst, share = R.within(name, key, got[key])
        print("%s %s: worst ratio %.2f of c = %d + %.1f (share %.3f)"
              % (name, key, worst, R.contraction(case, key), R.slack(name), share))
        if not ok or not bool(torch.isfinite(got[key]).all()):
            bad.append((key, worst))
    assert not bad, bad
    again = _run_kernel(case)                                   # the same bits
    for key in R.OUTPUTS:
        assert torch.equal(got[key].view(torch.int32), again[key].view(torch.int32)), key
    if name == "zero-rel":                                      # exact zeros, not small numbers
        assert float(got["dWrel"].abs().max()) == 0.0 and float(got["dbrel"].abs().max()) == 0.0


# ------------------------------------------------------------------------------ the tape
def _setup():
    if "head" not in _S:
        assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
        from pairnet_amd import PSGTr2HeadGrad, PSGTrHead2
        _, sd, _ = oracle_psgtr2_head(1234)
        head = PSGTrHead2(**psgtr2_cfg())
        head.load_state_dict(sd)
        head.to(DEV)
        head.exact_mask_order = True
        feats = [f.to(DEV) for f in seeded.seeded_feats(99, 2, H, W)]
        metas = [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)] * 2
        cls, masks = head.forward(feats, metas)
        torch.cuda.synchronize()
        pl = head._last_plan
        keep = {k: v.clone() for k, v in list(cls.items()) + list(masks.items())}
        tape = PSGTr2HeadGrad(head)
        out = tape.forward_from_plan(pl, with_mask=True)
        torch.cuda.synchronize()
        _S["head"] = dict(head=head, sd=sd, cls=cls, masks=masks, pl=pl, keep=keep, tape=tape,
                          out=out, feats=feats, metas=metas)
    return _S["head"]


def _random_grads(pl, counts, seed, fail=()):
    """Random upstream gradients in the loss's compact form; `fail`: images whose rows are -1 and
    whose mask-gradient rows hold NaN (they must not be read)."""
    B, Q = len(counts), 100
    g = torch.Generator().manual_seed(seed)
    grads = dict(sub=torch.randn(1, B, Q, 134, generator=g), obj=torch.randn(1, B, Q, 134, generator=g),
                 rel=torch.randn(1, B, Q, 57, generator=g))
    rows = torch.cat([torch.randperm(Q, generator=g)[:n].sort()[0] + b * Q
                      for b, n in enumerate(counts)]).long()
    M = rows.numel()
    both = torch.randn(2, M, pl.hw2[0], pl.hw2[1], generator=g)
    o = 0
    for b, n in enumerate(counts):
        if b in fail:
            rows[o:o + n] = -1
            both[:, o:o + n] = float("nan")
        o += n
    both = both.to(DEV)                       # one buffer, as the loss allocates it
    grads = {k: v.to(DEV) for k, v in grads.items()}
    grads.update(mask_rows=rows.to(DEV), sub_mask=both[0], obj_mask=both[1])
    return grads


def _reference(tape, pl, sd, grads, dtype=torch.float64, tape_gates=None):
    """Float64 autograd of the functional through the oracle's nine decoder layers (under the
    tape's mask bits) and the statement's heads -> (d mem, d MF, oracle head with .grad)."""
    head_o = OraclePSGTrHead2(**psgtr2_cfg()).eval()
    head_o.load_state_dict({k: v.detach().cpu() for k, v in sd.items()}, strict=True)
    head_o = head_o.to(dtype)               # (`dtype`: fp32 for the oracle's own miss, `_fp32_miss`)
    B, Q = pl.B, tape.Q
    if tape_gates is not None:              # a list: the FFN ReLUs under the tape's gates, flips noted
        from test_grad_gpu import _use_tape_ffn_gates
        _use_tape_ffn_gates(head_o, tape, B, Q, tape_gates)
    mem = pl.X.cpu().to(dtype).requires_grad_()
    MF = pl.MF.view(B, pl.HW2, 256).cpu().to(dtype).requires_grad_()
    keys, key_pos = [], []
    for l in range(3):
        h, w = pl.shapes[l]
        m = mem[:, pl.start[l]:pl.start[l] + pl.N[l]].transpose(0, 1)
        keys.append(m + head_o.level_embed.weight[l].view(1, 1, -1))
        pad = torch.zeros((B, h, w), dtype=torch.bool)
        key_pos.append(head_o.decoder_positional_encoding(pad).flatten(2).permute(2, 0, 1).to(dtype))
    q = head_o.query_feat.weight.unsqueeze(1).repeat((1, B, 1))
    q_pos = head_o.query_embed.weight.unsqueeze(1).repeat((1, B, 1))
    for i, layer in enumerate(head_o.transformer_decoder.layers):
        s = tape.dt["layers"][i]
        l = i % 3
        mask = _unpack_mask(s["bits"], s["rowall"], B, Q, pl.N[l])
        mask = mask.unsqueeze(1).repeat((1, head_o.n_heads, 1, 1)).flatten(0, 1)
        q = layer(query=q, key=keys[l], value=keys[l], query_pos=q_pos, key_pos=key_pos[l],
                  attn_masks=[mask, None], query_key_padding_mask=None, key_padding_mask=None)
    out = R.heads(q.transpose(0, 1), head_o.query_feat.weight, MF, dict(head_o.named_parameters()))
    c = lambda k: grads[k].cpu().to(dtype)
    R.functional(out, c("sub"), c("obj"), c("rel"), c("sub_mask"), c("obj_mask"),
                 grads["mask_rows"].cpu()).backward()
    return mem.grad, MF.grad, head_o


def test_taped_forward_equals_the_inference_forward():
    s = _setup()
    out, keep = s["out"], s["keep"]
    assert out["sub"].shape == (1, 2, 100, 134) and out["rel"].shape == (1, 2, 100, 57)
    assert out["me"].shape == (400, 256) and out["sub_seg"].shape == keep["sub_seg"].shape
    for k in ("sub", "obj", "rel", "sub_seg", "obj_seg"):
        err = float((out[k] - keep[k]).abs().max())
        print("taped %s: %.2e (max |.| %.2f)" % (k, err, float(keep[k].abs().max())))
        assert err < 1e-4, (k, err)
    # the replay left the caller's outputs alone
    for k, v in list(s["cls"].items()) + list(s["masks"].items()):
        assert torch.equal(v, keep[k]), k


@pytest.mark.parametrize("fail", [(), (1,)], ids=["clean", "image-1-failed"])
def test_backward_against_float64_autograd(fail):
    from pairnet_amd import PSGTr2HeadGrad
    s = _setup()
    head, tape, pl, sd = s["head"], s["tape"], s["pl"], s["sd"]
    grads = _random_grads(pl, COUNTS, seed=21 + len(fail), fail=fail)
    ends = []
    dmem, dMF, g = tape.backward(grads, counts=COUNTS, on_ready=ends.append)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tape.flat_grad).all()) and bool(torch.isfinite(dMF).all())
    dmem_ref, dMF_ref, head_o = _reference(tape, pl, sd, grads)
    names = [n for _, ns in PSGTr2HeadGrad.param_groups(head) for n in ns]
    assert len(names) == 179 and sorted(g) == sorted(names)
    report = []
    _compare("memory tokens", dmem, dmem_ref, report)
    _compare("mask feature", dMF, dMF_ref, report)
    _compare_params(g, head_o, report, names)
    _print(report)
    for n in R.UNREACHED:                                # autograd leaves them alone, and so does the tape
        assert dict(head_o.named_parameters())[n].grad is None and n not in g
    # flat layout: views of one buffer, segments on multiples of 64 floats, on_ready ends monotone
    lo = tape.flat_grad.data_ptr()
    for n, (off, shape, numel) in tape.layout.items():
        assert g[n].data_ptr() == lo + 4 * off and tuple(g[n].shape) == shape and off % 64 == 0
    assert ends == sorted(ends) and ends[-1] == tape.flat_numel == tape.size_of(head)
    assert ends[0] == tape.group_end["heads"] and len(ends) == 12
    # a second backward gives the same bits
    keep = (dmem.clone(), dMF.clone(), tape.flat_grad.clone())
    dmem2, dMF2, _ = tape.backward(grads, counts=COUNTS)
    torch.cuda.synchronize()
    assert torch.equal(dmem2, keep[0]) and torch.equal(dMF2, keep[1])
    assert torch.equal(tape.flat_grad.view(torch.int32), keep[2].view(torch.int32))
    if not fail:
        # two separately allocated mask gradients (the one copy) give the same bits as the halves
        sep = dict(grads, sub_mask=grads["sub_mask"].clone(), obj_mask=grads["obj_mask"].clone())
        dmem3, dMF3, _ = tape.backward(sep, counts=COUNTS)
        torch.cuda.synchronize()
        assert torch.equal(dMF3, keep[1]) and torch.equal(tape.flat_grad, keep[2])


def test_refusals():
    from pairnet_amd import PSGTr2HeadGrad
    s = _setup()
    head, tape, pl = s["head"], s["tape"], s["pl"]
    grads = _random_grads(pl, COUNTS, seed=1)
    with pytest.raises(RuntimeError):
        PSGTr2HeadGrad(head).backward(grads, counts=COUNTS)            # before forward_from_plan
    bad = [dict(grads, sub=grads["sub"][:, :1]), dict(grads, rel=grads["obj"]),
           dict(grads, sub_mask=grads["sub_mask"][:, :-1]), dict(grads, obj=grads["obj"].double()),
           dict(grads, mask_rows=grads["mask_rows"][:-1]), dict(grads, obj_mask=grads["obj_mask"].cpu()),
           {k: v for k, v in grads.items() if k != "obj_mask"}, dict(grads, cls=grads["sub"])]
    for i, gb in enumerate(bad):
        with pytest.raises(ValueError):
            tape.backward(gb, counts=COUNTS)
            pytest.fail("grads %d were accepted" % i)
    for counts in ([3, 2], [4], None, [3, 1, 0]):
        with pytest.raises(ValueError):
            tape.backward(grads, counts=counts)
