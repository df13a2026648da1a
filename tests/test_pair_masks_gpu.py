"""GPU: the subject / object result masks straight from the mask logits.

`pn_pair_masks_u8` (csrc/resize.hip, k_pair_masks) against the launch pair it replaces,
`hip.gather_rows` followed by `hip.bilinear_planar_gt0` -- `torch.equal`, no tolerance: on
every store width (16, 4, 1 columns per thread), staged in LDS and not, up- and downsampling,
one and several row strips, an output base 4 bytes off 16-byte alignment, and the index
patterns that decide which workgroup stores where (one object for all slots, a permutation,
objects named by one side only or by nobody, clamped indices, sub_pos == obj_pos).  The output
is pre-filled with 0xFF (every byte is 0 or 1 afterwards) and a guard row behind it stays 0xFF.

Then `CrossHead2` end to end with `fused_pair_masks` on and off, eagerly and through the
captured graphs, and `forward()`'s gathered logits; and `pn_resize_kept_f32`'s strip form
against the per-pixel-block form it replaces, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _logits(Q, hi, wi, seed):
    """Seeded logits centred on 0: both mask values occur."""
    return torch.randn(Q, hi * wi, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _reference(hip, mp, sub, obj, Q, R, hi, wi, ho, wo):
    seg = torch.empty(2 * R, hi * wi, device=DEV)
    hip.gather_rows(mp, sub, seg[:R], 1, Q, R, hi * wi)
    hip.gather_rows(mp, obj, seg[R:], 1, Q, R, hi * wi)
    want = torch.full((2 * R, ho, wo), 0xFF, device=DEV, dtype=torch.uint8)
    hip.bilinear_planar_gt0(seg, want, 2 * R, hi, wi, ho, wo)
    return want


def _check(mp, sub, obj, Q, R, hi, wi, ho, wo, offset=0):
    from pairnet_amd import hip
    sub = torch.as_tensor(sub, dtype=torch.int64, device=DEV)
    obj = torch.as_tensor(obj, dtype=torch.int64, device=DEV)
    want = _reference(hip, mp, sub, obj, Q, R, hi, wi, ho, wo)
    n = 2 * R * ho * wo
    buf = torch.full((offset + n + wo + 64,), 0xFF, device=DEV, dtype=torch.uint8)
    assert buf.data_ptr() % 16 == 0
    got = buf[offset:offset + n].view(2 * R, ho, wo)
    hip.pair_masks(mp, sub, obj, got, Q, R, hi, wi, ho, wo)
    torch.cuda.synchronize()
    assert int(got.max()) <= 1, "a byte of the output was not written"
    assert torch.equal(got, want)
    if hi * wi > 1:
        assert 0 < int(want.sum()) < want.numel()      # both mask values occur
    assert bool((buf[:offset] == 0xFF).all()) and bool((buf[offset + n:] == 0xFF).all())


PATTERNS = {            # Q = 5, R = 7
    "one_object": ([3] * 7, [3] * 7),
    "permutation": ([4, 2, 0, 3, 1, 2, 4], [1, 0, 3, 4, 2, 0, 3]),
    "sides": ([0, 0, 1, 1, 0, 1, 0], [3, 3, 3, 3, 3, 3, 3]),      # 0, 1: sub only; 3: obj only;
    "clamped": ([-3, 7, 1, -3, 2, 7, 0], [7, -3, 7, 2, -3, 1, 4]),  # 2, 4: nobody
    "same": ([2, 4, 4, 0, 1, 3, 2], [2, 4, 4, 0, 1, 3, 2]),
}

SHAPES = [              # (hi, wi, ho, wo)
    (25, 42, 48, 80),   # 16 columns per thread
    (25, 42, 48, 84),   # 4
    (25, 42, 47, 79),   # 1
    (25, 42, 12, 20),   # downsampling: clamped taps, i1 == i0 at the borders
    (7, 9, 13, 20),
    (1, 1, 4, 16),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%dx%d" % s)
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_pair_masks_equal_gather_then_resize(shape, pattern):
    hi, wi, ho, wo = shape
    sub, obj = PATTERNS[pattern]
    _check(_logits(5, hi, wi, seed=hi * 100 + wo), sub, obj, 5, 7, hi, wi, ho, wo)


def test_pair_masks_production_counts_two_strips():
    """Q = R = 100, 50 x 84 -> 96 x 160: two row strips per object, every slot-list length."""
    Q = R = 100
    g = torch.Generator().manual_seed(5)
    sub = torch.randint(0, Q, (R,), generator=g)
    obj = torch.randint(0, Q, (R,), generator=g)
    _check(_logits(Q, 50, 84, seed=6), sub, obj, Q, R, 50, 84, 96, 160)


@pytest.mark.parametrize("offset", [4, 1])
def test_pair_masks_unaligned_output_takes_a_narrow_path(offset):
    """wo % 16 == 0, but the output starts 4 bytes (1 byte) behind a 16-byte boundary: 4-byte
    (byte) stores, the same bits."""
    sub, obj = PATTERNS["permutation"]
    _check(_logits(5, 25, 42, seed=11), sub, obj, 5, 7, 25, 42, 48, 80, offset=offset)


def test_pair_masks_rows_too_long_for_lds_are_read_in_place():
    """Three source rows of 5000 floats exceed the staging budget: the direct-load form."""
    sub, obj = PATTERNS["clamped"]
    _check(_logits(5, 3, 5000, seed=13), sub, obj, 5, 7, 3, 5000, 5, 32)


def test_pair_masks_many_strips_and_wide_rows():
    """More than 256 column groups in a row (a thread walks several) and many strips."""
    sub, obj = PATTERNS["sides"]
    _check(_logits(5, 9, 300, seed=14), sub, obj, 5, 7, 9, 300, 21, 4112)


def test_pair_masks_bad_arguments_are_refused():
    from pairnet_amd import hip
    lib = hip.lib()
    assert lib.pn_pair_masks_u8(None, None, None, None, 5, 7, 4, 4, 8, 8, None) == -1
    assert lib.pn_pair_masks_u8(16, 16, 16, 16, 0, 7, 4, 4, 8, 8, None) == -1
    assert lib.pn_pair_masks_u8(16, 16, 16, 16, 70000, 7, 4, 4, 8, 8, None) == -1
    assert lib.pn_pair_masks_u8(16, 16, 16, 16, 5, 1025, 4, 4, 8, 8, None) == -1     # 2R > 2048
    assert lib.pn_pair_masks_u8(16, 16, 16, 16, 5, 7, 0, 4, 8, 8, None) == -1
    assert lib.pn_pair_masks_u8(16, 16, 16, 16, 5, 7, 4, 4, 8, 0, None) == -1
    assert lib.pn_resize_kept_f32(None, None, None, 5, 4, 4, 8, 8, 1, None) == -1
    assert lib.pn_resize_kept_f32(16, 16, 16, 5, 4, 4, 8, 8, 2, None) == -1
    assert lib.pn_resize_kept_f32(16, 16, 16, 257, 4, 4, 8, 8, 1, None) == -1


# ------------------------------------------------------------------ the head, end to end
@pytest.fixture(scope="module")
def head_and_feats():
    from helpers import head_cfg, oracle_head
    from pairnet_amd import CrossHead2
    _, sd, _ = oracle_head(1234)
    head = CrossHead2(**head_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    H, W = 96, 128
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(1, c, H // s, W // s, generator=g).to(DEV)
             for c, s in zip((256, 512, 1024, 2048), (4, 8, 16, 32))]
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4)]
    return head, feats, metas


def _poison(head, masks=None):
    """What an earlier run left in the plan's persistent buffers must not be able to pass for
    this run's output: NaN into the gathered logits, 0xFF into the result masks."""
    pl = getattr(head, "_last_plan", None)
    if pl is not None:
        pl.sub_seg.fill_(float("nan"))
        pl.obj_seg.fill_(float("nan"))
    if masks is not None:
        masks.view(torch.uint8).fill_(0xFF)
    torch.cuda.synchronize()


def _results(head, feats, metas, calls):
    """The last of `calls` calls (the first only makes the buffers known, so that every later one
    starts from poisoned ones; with graphs the third and fourth are replays)."""
    r = None
    for _ in range(calls):
        _poison(head, None if r is None else r[3])
        r = head.simple_test_bboxes(feats, metas)[0]     # (quiet here: graphs may be captured)
    torch.cuda.synchronize()
    return r, [t.clone() for t in r if torch.is_tensor(t)]


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_head_results_equal_with_the_switch_on_and_off(head_and_feats, graphs):
    """The fused run comes first and every run starts from poisoned buffers: its masks are
    what pn_pair_masks_u8 wrote in THIS call (every byte 0 / 1), and the gathered logits it did
    not need are still NaN afterwards -- the old path would have thresholded NaN to all-zero
    masks."""
    head, feats, metas = head_and_feats
    head.use_graphs = graphs
    res = {}
    for fused in (True, False):
        head.fused_pair_masks = fused
        live, res[fused] = _results(head, feats, metas, 4 if graphs else 2)
        pl = head._last_plan
        assert (pl.graph_b is not None) == graphs
        assert int(live[3].view(torch.uint8).max()) <= 1          # every byte written
        # the switch decides whether stage B gathers the mask logits
        assert bool(torch.isnan(pl.sub_seg).all()) == fused
        assert bool(torch.isnan(pl.obj_seg).all()) == fused
    assert len(res[True]) == len(res[False]) >= 6
    for a, b in zip(res[True], res[False]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    masks = res[True][3]
    assert masks.dtype == torch.bool and 0 < int(masks.sum()) < masks.numel()


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_forward_still_returns_the_gathered_logits(head_and_feats, graphs):
    head, feats, metas = head_and_feats
    head.use_graphs = graphs
    head.fused_pair_masks = True
    for _ in range(3 if graphs else 1):
        _poison(head)                        # nothing an earlier forward gathered survives
        _, masks = head.forward(feats, metas)
    torch.cuda.synchronize()
    sub_pos, obj_pos = head.pair_positions()
    mp = masks["mask"][0]
    assert not bool(torch.isnan(mp).any())
    assert torch.equal(masks["sub_seg"][0], mp[sub_pos[0]])
    assert torch.equal(masks["obj_seg"][0], mp[obj_pos[0]])
    assert len(set(sub_pos[0].tolist()) | set(obj_pos[0].tolist())) > 1


# ------------------------------------------------------------------ k_resize_kept
@pytest.mark.parametrize("nkeep", [0, 1, 9])
@pytest.mark.parametrize("shape", [(25, 42, 47, 79), (7, 9, 13, 20), (3, 5, 5, 4100)],
                         ids=lambda s: "%dx%d_%dx%d" % s)
def test_resize_kept_strip_form_equals_block_form(nkeep, shape):
    from pairnet_amd import hip
    Q = 9
    hi, wi, ho, wo = shape
    mp = _logits(Q, hi, wi, seed=nkeep + wo)
    state = torch.zeros(hip.panoptic_state_bytes() // 4, dtype=torch.int32)
    state[0] = nkeep
    state[16:16 + nkeep] = torch.randperm(Q, generator=torch.Generator().manual_seed(3))[:nkeep] \
        .to(torch.int32)
    state = state.to(DEV).view(torch.uint8)
    ups = []
    for form in (0, 1):
        up = torch.full((Q + 1, ho * wo), -7.0, device=DEV)
        hip.resize_kept(mp, up, state, Q, hi, wi, ho, wo, form=form)
        ups.append(up)
    torch.cuda.synchronize()
    assert torch.equal(ups[0], ups[1])
    assert bool((ups[1][nkeep:] == -7.0).all())
    if nkeep:
        assert not bool((ups[1][:nkeep] == -7.0).any())
