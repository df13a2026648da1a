"""Host: the float64 statement of the relation stage (tests/rel_grad_ref.py) is pinned to
`OracleCrossHeadBaseline.forward`, and the parameter names autograd reaches through it are exactly
the ones `BaselineHeadGrad` claims for the relation branch."""
import torch

import rel_grad_ref as RR
from helpers import baseline_cfg, oracle_baseline_head
from oracle import seeded

H, W = 64, 96
_S = {}


def _setup():
    if not _S:
        head_o, sd, _ = oracle_baseline_head(1234)
        head_o = head_o.double()
        feats = [f.double() for f in seeded.seeded_feats(99, 2, H, W)]
        mem, q, level = RR.trunk(head_o, feats)
        _S.update(head=head_o, feats=feats, mem=mem, q=q, level=level)
    return _S


def test_statement_equals_the_oracle_forward_in_float64():
    s = _setup()
    cls, _ = s["head"].forward(s["feats"], [dict(img_shape=(H, W, 3), scale_factor=[1.5] * 4)] * 2)
    with torch.no_grad():
        rel, sub, obj = RR.relation_stage(s["head"], s["mem"], s["q"], *s["level"])
    for name, got in (("rel", rel), ("subject_scores", sub), ("object_scores", obj)):
        assert got.dtype == torch.float64 and got.shape == cls[name].shape
        err = float((got - cls[name]).abs().max())
        print("%s: max |statement - oracle| = %.2e (max |.| %.2f)"
              % (name, err, float(cls[name].abs().max())))
        assert err <= 1e-12, (name, err)
    assert rel.shape == (2, 100, 57) and sub.shape == obj.shape == (2, 100, 100)


def test_autograd_reaches_exactly_the_names_the_tape_claims():
    from pairnet_amd import BaselineHeadGrad, CrossHeadBaseline, SegmenterHeadGrad
    s = _setup()
    grads, dmem, dq = RR.reached(s["head"], s["mem"], s["q"], s["level"])
    head = CrossHeadBaseline(**baseline_cfg())
    groups = BaselineHeadGrad.param_groups(head)
    parent = SegmenterHeadGrad.param_groups(head)
    assert groups[len(groups) - len(parent):] == parent          # the new groups come first
    claimed = [n for _, names in groups[:len(groups) - len(parent)] for n in names]
    assert len(claimed) == len(set(claimed)) == 2 + 2 * 4 + 6 * 18 + 2
    # the relation stage alone: the claimed names, plus level_embed through the keys
    assert set(grads) == set(claimed) | {"level_embed.weight"}
    assert all(grads[n] is not None and float(grads[n].abs().max()) > 0 for n in claimed)
    assert float(dmem.abs().max()) > 0 and float(dq.abs().max()) > 0
    # every relation-branch parameter of the head is claimed, and nothing else is
    shapes = head.param_shapes()
    branch = [k for k in shapes if k.startswith(RR.REL_PREFIXES)]
    assert sorted(set(branch) - set(claimed)) == sorted(RR.UNREACHABLE)   # no .grad there: unused
    assert set(claimed) <= set(branch) and not set(RR.UNREACHABLE) & set(grads)
    assert all(tuple(shapes[k]) == tuple(grads[k].shape) for k in claimed)
    # the whole tape: every head parameter except the pixel decoder's
    every = [n for _, names in groups for n in names]
    assert len(every) == len(set(every))
    assert set(every) == {k for k in shapes if not k.startswith("pixel_decoder.")} - set(RR.UNREACHABLE)
    assert BaselineHeadGrad.size_of(head) == sum((int(torch.Size(shapes[n]).numel()) + 63) // 64 * 64
                                                 for n in every)


def test_the_entry_is_declared_bound_and_built():
    import os
    import re
    from pairnet_amd import build as B, hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pairnet_hip.h")).read()
    for name in ("pn_mha_bwd_keysplit_f32", "pn_mha_bwd_keysplit_scratch_floats",
                 "pn_mha_keysplit_chunk"):
        assert name in hip._SIGS and name in hip.EXPORTS and re.search(r"\b%s\(" % name, header)
    assert "attn_grad" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "attn_grad.hip"))
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION == 34
    src = open(os.path.join(B.CSRC, "attn_grad.hip")).read()
    assert int(re.search(r"#define KS_CHUNK (\d+)", src).group(1)) == hip.MHA_KEYSPLIT_CHUNK
    assert "atomic" not in src.replace("No atomics", "").replace("no atomics", "")
    assert callable(hip.mha_bwd_keysplit) and callable(hip.mha_bwd_keysplit_scratch_floats)
