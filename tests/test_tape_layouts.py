"""CPU: the flat layout of every backward tape is the checkpoint format (`runner.save_checkpoint`
stores the AdamW moments in flat order, and `dist.GradReducer` is handed the groups' ends), so the
ordered (group, names) list and `size_of` of all eleven tape classes are pinned to
tests/golden/tape_layouts.json.  That fixture was written from the commit BEFORE the tapes got
their common base (`Tape`, pair-net_amd/tape.py), through the public names only:

    cd tests && PYTHONPATH=.. python -c "import json, test_tape_layouts as t; \
        json.dump(t._layouts(), open('golden/tape_layouts.json', 'w'), indent=0, sort_keys=True)"

`param_groups` and `size_of` are static and need no GPU."""
import json
import os

import pytest

from helpers import GOLDEN, baseline_cfg, head_cfg, psgtr2_cfg

SWIN_DIMS = dict(embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), window_size=7)
HEAD_TAPES = ("RelationTailGrad", "HeadGrad", "BBoxTailGrad", "SegmenterHeadGrad",
              "BaselineHeadGrad", "PSGTr2HeadGrad")
BACKBONE_TAPES = ("PixelDecoderGrad", "BackboneGrad", "SwinBackboneGrad", "SwinStagesGrad")
TAPES = HEAD_TAPES + BACKBONE_TAPES + ("SegPixelDecoderGrad",)


def _modules():
    """Tape class name -> the module it tapes, on the tests' small configurations."""
    import pairnet_amd as P
    head = P.CrossHead2(**head_cfg())
    base = P.CrossHeadBaseline(**baseline_cfg())
    tri = P.PSGTrHead2(**psgtr2_cfg())
    box = P.CrossHeadBBox(**{k: v for k, v in P.bbox_head_cfg().items() if k != "type"})
    return {"RelationTailGrad": head, "HeadGrad": head, "PixelDecoderGrad": head,
            "BBoxTailGrad": box, "SegmenterHeadGrad": base, "BaselineHeadGrad": base,
            "SegPixelDecoderGrad": base, "PSGTr2HeadGrad": tri,
            "BackboneGrad": P.ResNet50Hip(),
            "SwinBackboneGrad": P.SwinTransformerHip(frozen_stages=3, **SWIN_DIMS),
            "SwinStagesGrad": P.SwinTransformerHip(frozen_stages=-1, **SWIN_DIMS)}


def _layouts():
    import pairnet_amd as P
    out = {}
    for name, module in _modules().items():
        cls = getattr(P, name)
        out[name] = dict(groups=[[g, list(ns)] for g, ns in cls.param_groups(module)],
                         size_of=int(cls.size_of(module)))
    return out


@pytest.fixture(scope="module")
def layouts():
    return _layouts()


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "tape_layouts.json")) as f:
        return json.load(f)


def test_the_fixture_covers_the_eleven_tapes(want, layouts):
    assert len(TAPES) == 11 and set(want) == set(TAPES) == set(layouts)


@pytest.mark.parametrize("name", TAPES)
def test_tape_layout_is_the_checkpoint_format(layouts, want, name):
    got, ref = layouts[name], want[name]
    assert [g for g, _ in got["groups"]] == [g for g, _ in ref["groups"]]
    assert got["groups"] == ref["groups"]
    assert got["size_of"] == ref["size_of"]


def test_every_tape_is_a_tape_and_only_the_head_tapes_are_tails():
    import pairnet_amd as P
    from pairnet_amd.tape import Tape
    for name in TAPES:
        assert issubclass(getattr(P, name), Tape), name
    for name in BACKBONE_TAPES:
        assert not issubclass(getattr(P, name), P.RelationTailGrad), name
    assert issubclass(P.SegPixelDecoderGrad, P.PixelDecoderGrad)
    assert not issubclass(P.SegPixelDecoderGrad, P.RelationTailGrad)
