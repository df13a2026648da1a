"""CPU: what `PSGTr2HeadGrad`, `PSGTr2Trainer` and `pn_triplet_heads_bwd_f32` promise without a GPU
-- the float64 statement of the head chain (tests/tri_grad_ref.py) reproduces the reference-pinned
oracle's five outputs (the "sic" wiring); the tape's layout is exactly what autograd reaches through
that oracle; the layout's padding, order and size; the optimizer multipliers of
psgtr_r50_psg_plus.py; the kernel's bound function holds for torch's own fp32 result on every kernel
case; the entry is declared, bound and built and refuses what it cannot take."""
import ctypes
import os
import re

import pytest
import torch

import tri_grad_ref as R
from helpers import oracle_psgtr2_head, psgtr2_cfg
from oracle import seeded
from oracle.psgtr_head2 import OraclePSGTrHead2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 64, 96
_S = {}


def _oracle_run():
    """The oracle head in float64 on the 64 x 96 pyramid, 2 images, autograd on: its five outputs,
    the last decoder layer's output and the mask feature (through hooks), and the head."""
    if "run" not in _S:
        head_o, sd, _ = oracle_psgtr2_head(1234)
        head_o = head_o.double()
        for p in head_o.parameters():
            p.requires_grad_(True)
        feats = [f.double().requires_grad_() for f in seeded.seeded_feats(99, 2, H, W)]
        metas = [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)] * 2
        seen = {}
        h1 = head_o.transformer_decoder.layers[-1].register_forward_hook(
            lambda m, i, o: seen.__setitem__("q_last", o))
        h2 = head_o.pixel_decoder.register_forward_hook(
            lambda m, i, o: seen.__setitem__("MF", o[0]))
        try:
            cls, masks = OraclePSGTrHead2.forward.__wrapped__(head_o, feats, metas)
        finally:
            h1.remove()
            h2.remove()
        _S["run"] = (head_o, feats, cls, masks, seen)
    return _S["run"]


def test_statement_equals_the_oracles_five_outputs():
    head_o, _, cls, masks, seen = _oracle_run()
    p = {k: v.detach() for k, v in head_o.named_parameters()}
    q_last = seen["q_last"].detach().transpose(0, 1)                      # [B, Q, 256]
    MF = seen["MF"].detach().flatten(2).transpose(1, 2)                   # [B, P, 256]
    sub, obj, rel, sub_seg, obj_seg = R.heads(q_last, p["query_feat.weight"], MF, p)
    h, w = masks["sub_seg"].shape[-2:]
    for name, got, want in (("sub", sub, cls["sub"][0]), ("obj", obj, cls["obj"][0]),
                            ("rel", rel, cls["rel"][0]),
                            ("sub_seg", sub_seg.view(2, -1, h, w), masks["sub_seg"][0]),
                            ("obj_seg", obj_seg.view(2, -1, h, w), masks["obj_seg"][0])):
        err = float((got - want.detach()).abs().max())
        print("%s: %.2e (max |.| %.2f)" % (name, err, float(want.detach().abs().max())))
        assert got.dtype == torch.float64 and err <= 1e-12, (name, err)
    # the two mask outputs differ: they are the same MLP on two different query sets
    assert float((sub_seg - obj_seg).abs().max()) > 1e-3


def test_layout_is_what_autograd_reaches_through_the_oracle():
    from pairnet_amd import PSGTr2HeadGrad, PSGTrHead2, SegPixelDecoderGrad
    head_o, feats, cls, masks, _ = _oracle_run()
    g = torch.Generator().manual_seed(5)
    F = sum((t * torch.randn(t.shape, generator=g, dtype=torch.float64)).sum()
            for t in list(cls.values()) + list(masks.values()))
    for p in head_o.parameters():
        p.grad = None
    F.backward(retain_graph=True)
    every = dict(head_o.named_parameters())
    reached = {n for n, p in every.items() if p.grad is not None}
    assert len(every) == 308 and len(reached) == 296
    assert sum(every[n].numel() for n in reached) == 20578053
    assert sorted(set(every) - reached) == sorted(R.UNREACHED)
    assert all(f.grad is not None and float(f.grad.abs().max()) > 0 for f in feats)
    head = PSGTrHead2(**psgtr2_cfg())
    names = [n for _, ns in PSGTr2HeadGrad.param_groups(head) for n in ns]
    assert len(names) == len(set(names)) == 179
    assert set(names) == {n for n in reached if not n.startswith("pixel_decoder.")}
    assert set(R.HEAD_PARAMS) <= set(names) and not set(R.UNREACHED) & set(names)
    pd = {n for _, ns in SegPixelDecoderGrad.param_groups(head) for n in ns}
    assert pd == {n for n in reached if n.startswith("pixel_decoder.")} and len(pd) == 117


def test_layout_padding_order_and_size():
    from pairnet_amd import PSGTr2HeadGrad, PSGTrHead2
    head = PSGTrHead2(**psgtr2_cfg())
    groups = PSGTr2HeadGrad.param_groups(head)
    assert [g for g, _ in groups] == ["heads"] + ["transformer_decoder.layers.%d" % i
                                                 for i in reversed(range(9))] + ["query"]
    assert set(groups[0][1]) == set(R.HEAD_PARAMS)
    assert groups[-1][1] == ["query_feat.weight", "query_embed.weight", "level_embed.weight"]
    want = sum((head._params[n].numel() + 63) // 64 * 64 for _, ns in groups for n in ns)
    assert PSGTr2HeadGrad.size_of(head) == want and want % 64 == 0
    # (the offsets themselves -- every segment on a multiple of 64 floats -- are built by the same
    # `_build_layout` as every tape's: checked on the device in tests/test_tri_grad_gpu.py)
    assert issubclass(PSGTr2HeadGrad, __import__("pairnet_amd").SegmenterHeadGrad)


def test_optimizer_multipliers_of_the_config():
    from pairnet_amd import BaselineTrainer, PSGTr2Trainer
    from pairnet_amd.baseline_train import CUSTOM_KEYS
    import inspect
    sig = inspect.signature(PSGTr2Trainer.__init__).parameters
    assert (sig["lr"].default, sig["weight_decay"].default, sig["max_norm"].default) == (1e-4, 1e-4, 0.1)
    assert sig["norm_decay_mult"].default == 1.0 and sig["deterministic"].default is False
    assert sig["masked_keysplit_min_keys"].default == "default"
    assert PSGTr2Trainer.MASKED_KEYSPLIT_MIN_KEYS == BaselineTrainer.MASKED_KEYSPLIT_MIN_KEYS
    assert (PSGTr2Trainer.LR_STEPS, PSGTr2Trainer.LR_GAMMA) == ((40,), 0.1)
    lr, dm = {k: 0.1 for k in CUSTOM_KEYS}, {k: 1.0 for k in CUSTOM_KEYS}
    m = lambda n: BaselineTrainer.multipliers(n, lr, dm, 1.0)
    assert m("backbone.layer3.0.conv1.weight") == (0.1, 1.0)
    assert m("transformer_decoder.layers.4.norms.1.weight") == (0.1, 1.0)
    assert m("transformer_decoder.post_norm.bias") == (0.1, 1.0)
    assert m("pixel_decoder.input_convs.0.gn.weight") == (0.1, 1.0)
    assert m("sub_cls_embed.weight") == (1.0, 1.0)
    assert m("obj_mask_embed.0.bias") == (1.0, 1.0)
    assert m("query_feat.weight") == (1.0, 1.0)
    assert "UNPINNED" in __import__("pairnet_amd.psgtr2_train", fromlist=["x"]).__doc__


@pytest.mark.parametrize("name", list(R.CASES))
def test_bound_holds_for_torch_fp32_on_every_kernel_case(name):
    case = R.kernel_case(name)
    a = R.slack(name)
    t32 = R.kernel_torch32(case)
    assert a >= 4.0
    for key in R.OUTPUTS:
        ok, worst, share = R.within(name, key, t32[key])
        print("%s %s: torch fp32 worst ratio %.2f, c %d + %.1f, share %.3f"
              % (name, key, worst, R.contraction(case, key), a, share))
        assert ok, (name, key, worst)
    if name == "zero-rel":
        ref = R.kernel_ref64(case)
        assert float(ref["dWrel"].abs().max()) == 0.0 and float(ref["dbrel"].abs().max()) == 0.0
        assert float(ref["dWsub"].abs().max()) > 0
    assert case["add"] == (name == "add")


def test_entry_is_declared_bound_built_and_refuses(built_lib):
    from pairnet_amd import api, build as B, hip
    header = open(os.path.join(ROOT, "include", "pairnet_hip.h")).read()
    name = "pn_triplet_heads_bwd_f32"
    assert name in hip._SIGS and name in hip.EXPORTS and re.search(r"\b%s\(" % name, header)
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION == 34
    assert "tri_grad" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "tri_grad.hip"))
    src = open(os.path.join(B.CSRC, "tri_grad.hip")).read()
    assert "atomic" not in src.replace("no float atomics", "") and "mfma32(" in src
    lib = ctypes.CDLL(B.LIB_PATH)
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = hip._SIGS[name]
    one = ctypes.c_void_p(64)               # (never dereferenced: every call below is refused first)
    ok = [one] * 14 + [200, 256, 134, 57, 1, None]
    for i, v in ((14, 0), (14, 4097), (15, 128), (16, 257), (16, 0), (17, 65), (17, 0), (18, 2),
                 (0, None), (7, None), (13, None)):
        args = list(ok)
        args[i] = v
        assert fn(*args) == -1, (i, v)
    # the wrapper's limits, in the project's NotImplementedError form, before any pointer is taken
    z = lambda *s: torch.zeros(*s)
    def call(N=8, C1=5, Cr1=3, ch=256):
        hip.tri_heads_bwd(z(N, C1), z(N, C1), z(N, Cr1), z(N, ch), z(C1, ch), z(C1, ch), z(Cr1, ch),
                          z(N, ch), z(C1, ch), z(C1), z(C1, ch), z(C1), z(Cr1, ch), z(Cr1))
    for kw, text in ((dict(ch=128), "256 channels"), (dict(N=4097), "<= 4096 rows"),
                     (dict(C1=257), r"C \+ 1 <= 256"), (dict(Cr1=65), r"Cr \+ 1 <= 64")):
        with pytest.raises(NotImplementedError, match=text):
            call(**kw)
    with pytest.raises(RuntimeError, match="device tensors"):
        call()
    for n in ("PSGTr2HeadGrad", "PSGTr2Trainer"):
        assert n in api.__all__ and hasattr(api, n)
    from pairnet_amd import CrossHead2, PSGTr, PSGTr2Trainer
    from helpers import head_cfg
    assert callable(PSGTr.triplet_trainer) and callable(PSGTr.triplet_train_step)
    with pytest.raises(NotImplementedError):
        PSGTr2Trainer(CrossHead2(**head_cfg()))
