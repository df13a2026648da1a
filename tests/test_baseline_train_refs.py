"""CPU: what `BaselineTrainer` and the masked key-split entry promise without a GPU -- the entry is
declared, bound and built; the optimizer-group rule (restated from memory of mmcv's
DefaultOptimizerConstructor: mmcv does not import here, so nothing pins it to mmcv); the public
names; the constructor's host-side refusals."""
import os
import re

import pytest
import torch

from helpers import baseline_cfg, head_cfg


def test_the_masked_entry_is_declared_bound_and_built(built_lib):
    import ctypes
    from pairnet_amd import build as B, hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pairnet_hip.h")).read()
    name = "pn_mha_bwd_keysplit_masked_f32"
    assert name in hip._SIGS and name in hip.EXPORTS and re.search(r"\b%s\(" % name, header)
    assert hasattr(ctypes.CDLL(B.LIB_PATH), name)
    old, new = hip._SIGS["pn_mha_bwd_keysplit_f32"], hip._SIGS[name]
    assert new[0] is old[0] and new[1][:-1] == old[1][:-1] + [ctypes.c_void_p] * 2   # + bits, rowall
    assert int(re.search(r"#define PN_ABI_VERSION (\d+)", header).group(1)) == hip.ABI_VERSION
    src = open(os.path.join(B.CSRC, "attn_grad.hip")).read()
    assert "atomic" not in src.replace("No atomics", "").replace("no atomics", "")
    import inspect
    sig = inspect.signature(hip.mha_bwd_keysplit)
    assert sig.parameters["bits"].default is None and sig.parameters["rowall"].default is None


def test_optimizer_group_rule():
    from pairnet_amd import BaselineTrainer
    keys = {k: 0.1 for k in ("backbone", "transformer_decoder", "pixel_decoder", "decoder_input_projs")}
    m = lambda n: BaselineTrainer.multipliers(n, keys, keys, 0.0)
    # a key hit takes the key's two multipliers and nothing else (a norm under a key decays at 0.1)
    assert m("transformer_decoder.layers.0.norms.0.weight") == (0.1, 0.1)
    assert m("transformer_decoder.post_norm.bias") == (0.1, 0.1)
    assert m("pixel_decoder.input_convs.1.gn.weight") == (0.1, 0.1)
    assert m("pixel_decoder.encoder.layers.2.ffns.0.layers.1.weight") == (0.1, 0.1)
    assert m("backbone.layer2.0.conv1.weight") == (0.1, 0.1)
    # a norm outside every key: norm_decay_mult
    assert m("relation_decoder.layers.5.norms.2.bias") == (1.0, 0.0)
    # everything else
    for n in ("rel_cls_embed.weight", "cls_embed.bias", "mask_embed.2.weight", "query_feat.weight",
              "level_embed.weight", "sub_query_update.0.weight",
              "relation_decoder.layers.0.attentions.1.attn.in_proj_weight"):
        assert m(n) == (1.0, 1.0), n
    # the longest key decides; a key given for one multiplier leaves the other at 1
    assert BaselineTrainer.multipliers("ab.c", {"ab": 0.5, "ab.c": 0.25}, {"ab": 0.0}, 0.0) == (0.25, 1.0)


def test_public_names_and_host_refusals():
    from pairnet_amd import api
    from pairnet_amd import (BaselineTrainer, CrossHead2, CrossHeadBaseline, PSGTr, SegmenterHeadGrad,
                             SwinTransformerHip, swin_backbone_cfg)
    assert "BaselineTrainer" in api.__all__ and api.BaselineTrainer is BaselineTrainer
    assert callable(PSGTr.full_trainer) and callable(PSGTr.full_train_step)
    with pytest.raises(NotImplementedError):
        BaselineTrainer(CrossHead2(**head_cfg()))
    swin = SwinTransformerHip(**{k: v for k, v in swin_backbone_cfg("T").items() if k != "type"})
    with pytest.raises(NotImplementedError):
        BaselineTrainer(CrossHeadBaseline(**baseline_cfg()), backbone=swin)
    assert BaselineTrainer.MASKED_KEYSPLIT_MIN_KEYS is None or \
        isinstance(BaselineTrainer.MASKED_KEYSPLIT_MIN_KEYS, int)
    import inspect
    assert "masked_keysplit_min_keys = None" in inspect.getsource(SegmenterHeadGrad.__init__)
