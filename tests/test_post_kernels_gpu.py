"""GPU: the kernels that decide -- labels, argmax indices, top-k lists, panoptic ids -- and the
glue of the box trunk, one exported entry at a time through the hip.* wrappers: csrc/postproc.hip
up to pn_pack_triplets_f32, the three top-k entries of csrc/ppn.hip, all of csrc/detr.hip and
pn_sine_pe_valid_f32, against the float64 / integer statements of tests/post_ref.py (pinned to
torch and the oracle without a GPU by tests/test_post_refs.py) on the inputs of tests/post_cases.py.

Decision outputs are integers and are compared exactly.  On decisive inputs (values on the 1/8
grid, exact ties, integer-valued masks resized 1:1) the answer is unique under the first-index
rule.  On random inputs an index is admissible if its float64 score is within the value bound of
the float64 winner; every output must be admissible, and exact where the float64 margin exceeds
the bound (test_post_refs.py shows that this is all but 1 % of the rows / pixels).

Value outputs are bounded element-wise: |got - ref| <= (L + a + cond) 2^-24 mag + FLT_MIN, with
L the chain of fp32 roundings counted from the kernel's source (the table is in labnotes/r22.md,
written before the first run, and beside each test), cond the roundings an exp / log / sin / cos /
pow multiplies, from the inputs alone (post_ref.py states each), a = max(4, 2 x the ratio torch's
own fp32 evaluation reaches on the same inputs).  Nothing in a bound comes from the kernel under
test.  Every case prints the kernel's and the fp32 oracle's ratio and c; the worst per kernel is
printed when the module ends.

Every output is allocated with spare rows / columns holding the NaN bit pattern, which the call
must leave alone; every kernel is launched twice and must give equal bits; every refusal of an
entry's argument check is tried once, must raise and must leave the outputs untouched."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fwd_cases
import fwd_ref
import post_cases as K
import post_ref as R
import test_fwd_kernels_gpu as FW
from test_fwd_kernels_gpu import _bounded as _fw_bounded, _d, _is_fence, _nan, _same_bits
from test_grad_kernels_gpu import FLT_MIN, U, _within  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FI32 = 0x7fc00000
FI64 = 0x7fc000007fc00000
MINE = set()


@pytest.fixture(scope="module")
def hip(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip as h
    h.lib()
    yield h
    print("\n%-26s %12s %14s %10s  case" % ("kernel", "worst ratio", "fp32 oracle", "c"))
    for k in sorted(MINE):
        r, o, c, case = FW.WORST[k]
        print("%-26s %12.3f %14.3f %10.4g  %s" % (k, r, o, c, case))


def _bounded(kernel, *args, **kw):
    MINE.add(kernel)
    return _fw_bounded(kernel, *args, **kw)


def _fi64(*shape):
    return torch.full(shape, FI64, device=DEV, dtype=torch.int64)


def _fi32(*shape):
    return torch.full(shape, FI32, device=DEV, dtype=torch.int32)


def _eq(a, b):
    return _same_bits(a, b) if a.is_floating_point() else torch.equal(a, b)


def _fence(t):
    if t.is_floating_point():
        return _is_fence(t)
    return bool((t == (FI64 if t.dtype == torch.int64 else FI32)).all())


def _twice(launch):
    """Runs `launch` (allocates fenced outputs, calls the kernel, returns them) twice; the two
    sets of outputs must have equal bits."""
    a = launch()
    b = launch()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert _eq(x, y), "not bitwise reproducible"
    return a


def _refused(calls, outs):
    """Every call must raise, and no output may change."""
    before = [o.clone() for o in outs]
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail("refusal %d was accepted" % i)
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert _eq(o, b)


def _i64(v):
    return torch.as_tensor(v, dtype=torch.int64, device=DEV)


# ============================================================ label / probability kernels
# L = 14 (post_ref.SOFT_L): exp on the numerator (2); exp (2), 3 in-lane adds and 6 shuffle adds
# on the denominator; the quotient.  cond = |d_i| + sum p |d| (post_ref.softmax).
def _cls_run(hip, x, off):
    rows, C = x.shape
    xd = _d(x)

    def launch():
        label, score = _fi64(rows + 3), _nan(rows + 3)
        hip.cls_argmax(xd, label, score, rows, C, off)
        return label, score
    label, score = _twice(launch)
    assert _fence(label[rows:]) and _fence(score[rows:])
    return label[:rows], score[:rows]


@pytest.mark.parametrize("C,rows,seed", K.soft_cases())
def test_post_cls_argmax(hip, C, rows, seed):
    x = K.soft_input(C, rows, seed)
    o32 = F.softmax(x, -1)[:, :C - 1].max(-1)[0]
    for off in (0, 1):
        want, ref, mag, cond, _ = R.cls_argmax(x, off)
        label, score = _cls_run(hip, x, off)
        assert torch.equal(label.cpu(), want), (label.cpu(), want)
        _bounded("k_cls_argmax", "C %d rows %d off %d" % (C, rows, off), score, ref, mag,
                 R.SOFT_L, o32, cond=cond)


@pytest.mark.parametrize("C", [2, 3, 65, 134, 256])
def test_post_cls_argmax_rows_without_a_softmax(hip, C):
    """All -inf, a +inf, a NaN: the score is NaN and the label is offset + the first NaN among
    the admitted logits (0 where there is none), always inside [offset, offset + C - 2]."""
    x, want = K.hostile_rows(C)
    for off in (0, 1):
        label, score = _cls_run(hip, x, off)
        assert torch.equal(label.cpu(), want + off), (label.cpu(), want + off)
        assert bool(torch.isnan(score).all())
        assert torch.equal(label.cpu(), R.cls_argmax(x, off)[0])


@pytest.mark.parametrize("C,rows,seed", K.SOFT_RANDOM)
def test_post_cls_argmax_random(hip, C, rows, seed):
    x = K.soft_random(C, rows, seed)
    p, mag, cond = R.softmax(x)
    bound, a = R.value_bound(p, mag, R.SOFT_L, cond, F.softmax(x, -1))
    label, score = _cls_run(hip, x, 1)
    got = label.cpu() - 1
    assert bool(((got >= 0) & (got <= C - 2)).all())
    adm, badm = p[:, :C - 1], bound[:, :C - 1]
    top, win = adm.max(-1)
    slack = badm.gather(1, got[:, None])[:, 0] + badm.gather(1, win[:, None])[:, 0]
    assert bool((top - adm.gather(1, got[:, None])[:, 0] <= slack).all()), "inadmissible label"
    rest = adm.clone()
    rest.scatter_(1, win[:, None], -1.0)
    clear = ((top[:, None] - rest) > (badm + badm.gather(1, win[:, None]))).all(-1)
    assert float(clear.double().mean()) >= 0.99
    assert torch.equal(got[clear], win[clear])
    pg = p.gather(1, got[:, None])[:, 0]
    _bounded("k_cls_argmax", "random C %d" % C, score, pg, pg, R.SOFT_L,
             F.softmax(x, -1).gather(1, got[:, None])[:, 0], cond=cond.gather(1, got[:, None])[:, 0])


@pytest.mark.parametrize("C,rows,seed", K.soft_cases(extra_c=(1,)))
def test_post_rel_dists(hip, C, rows, seed):
    x = K.soft_input(C, rows, seed, admitted=C)
    xd = _d(x)

    def launch():
        out = _nan((rows + 2) * (C + 1))
        hip.rel_dists(xd, out, rows, C)
        return (out,)
    out, = _twice(launch)
    assert _is_fence(out[rows * (C + 1):])
    out = out[:rows * (C + 1)].view(rows, C + 1)
    assert bool((out[:, 0].view(torch.int32) == 0).all()), "column 0 is not +0"
    ref, mag, cond = R.rel_dists(x)
    o32 = torch.cat([torch.zeros(rows, 1), F.softmax(x, -1)], -1)
    _bounded("k_rel_dists", "C %d rows %d" % (C, rows), out, ref, mag, R.SOFT_L, o32, cond=cond)


@pytest.mark.parametrize("C,rows,seed", K.soft_cases())
def test_post_softmax_fg(hip, C, rows, seed):
    x = K.soft_input(C, rows, seed, admitted=C)
    xd = _d(x)

    def launch():
        probs, fg = _nan((rows + 2) * C), _nan((rows + 2) * (C - 1) + 1)
        hip.softmax_fg(xd, probs, fg, rows, C)
        return probs, fg
    probs, fg = _twice(launch)
    assert _is_fence(probs[rows * C:]) and _is_fence(fg[rows * (C - 1):])
    probs, fg = probs[:rows * C].view(rows, C), fg[:rows * (C - 1)].view(rows, C - 1)
    assert _same_bits(fg, probs[:, 1:]), "fg is not probs[:, 1:] bit for bit"
    ref, mag, cond = R.softmax(x)
    _bounded("k_softmax_fg", "C %d rows %d" % (C, rows), probs, ref, mag, R.SOFT_L,
             F.softmax(x, -1), cond=cond)


@pytest.mark.parametrize("n", K.ARGMAX_N)
def test_post_row_argmax(hip, n):
    for rows in K.ARGMAX_ROWS:
        x = K.argmax_input(n, rows, n)
        xd = _d(x)

        def launch():
            idx = _fi64(rows + 3)
            hip.row_argmax(xd, idx, rows, n)
            return (idx,)
        idx, = _twice(launch)
        assert _fence(idx[rows:])
        assert torch.equal(idx[:rows].cpu(), R.argmax_first(x.numpy())), (n, rows)


def test_post_row_argmax_nan_is_pinned(hip):
    """The kernel's present behaviour on NaN, as its header states it: a NaN in a column >= 64
    is skipped, a NaN in column 0 gives 0 (torch would name the NaN's position in both cases)."""
    n = 129
    x = K.grid(K.gen(0), 3, n, lo=-32, hi=1)
    x[0, 70], x[0, 100] = math.nan, 2.0
    x[1, 0], x[1, 90] = math.nan, 2.0
    x[2, 128], x[2, 3] = math.nan, 2.0
    idx = _fi64(3)
    hip.row_argmax(_d(x), idx, 3, n)
    assert idx.tolist() == [100, 0, 3]


def test_post_label_refusals(hip):
    x = _d(K.soft_input(5, 4, 0))
    label, score, out = _fi64(8), _nan(8), _nan(64)
    _refused([
        lambda: hip.cls_argmax(None, label, score, 4, 5), lambda: hip.cls_argmax(x, None, score, 4, 5),
        lambda: hip.cls_argmax(x, label, None, 4, 5), lambda: hip.cls_argmax(x, label, score, 0, 5),
        lambda: hip.cls_argmax(x, label, score, 4, 1), lambda: hip.cls_argmax(x, label, score, 4, 257),
        lambda: hip.rel_dists(None, out, 4, 5), lambda: hip.rel_dists(x, None, 4, 5),
        lambda: hip.rel_dists(x, out, 0, 5), lambda: hip.rel_dists(x, out, 4, 0),
        lambda: hip.rel_dists(x, out, 4, 257),
        lambda: hip.softmax_fg(None, out, out, 4, 5), lambda: hip.softmax_fg(x, None, out, 4, 5),
        lambda: hip.softmax_fg(x, out, None, 4, 5), lambda: hip.softmax_fg(x, out, out, 0, 5),
        lambda: hip.softmax_fg(x, out, out, 4, 1), lambda: hip.softmax_fg(x, out, out, 4, 257),
        lambda: hip.row_argmax(None, label, 4, 5), lambda: hip.row_argmax(x, None, 4, 5),
        lambda: hip.row_argmax(x, label, 0, 5), lambda: hip.row_argmax(x, label, 4, 0),
    ], [label, score, out])


# ============================================================ triplet records: data movement
@pytest.mark.parametrize("k", [1, 100])
@pytest.mark.parametrize("C", [2, 57, 300])
def test_post_triplet_finish(hip, k, C):
    g = K.gen(k + C)
    nq = 7
    s_label, o_label = torch.randint(0, 133, (nq,), generator=g), torch.randint(0, 133, (nq,), generator=g)
    probs = torch.rand(nq, C, generator=g)
    tri = torch.randint(0, nq, (k,), generator=g)
    rem = torch.randint(0, C - 1, (k,), generator=g)
    ins = [_d(t) for t in (s_label, o_label, probs, tri, rem)]

    def launch():
        outs = _fi64(2 * k + 3), _fi64(k + 3), _nan(k + 3), _nan((k + 1) * C)
        hip.triplet_finish(*ins, *outs, k, C)
        return outs
    labels, r_labels, r_scores, r_dists = _twice(launch)
    assert _fence(labels[2 * k:]) and _fence(r_labels[k:]) and _fence(r_scores[k:]) and \
        _fence(r_dists[k * C:])
    assert torch.equal(labels[:2 * k].cpu(), torch.cat([s_label[tri] + 1, o_label[tri] + 1]))
    assert torch.equal(r_labels[:k].cpu(), rem + 1)
    assert _same_bits(r_scores[:k], _d(probs[tri, rem + 1]))
    assert _same_bits(r_dists[:k * C].view(k, C), _d(probs[tri]))
    if k == 1 and C == 2:
        a = ins
        o = [labels, r_labels, r_scores, r_dists]
        bad = []
        for i in range(9):                       # each of the nine pointers absent
            args = list(a) + o
            args[i] = None
            bad.append(lambda args=args: hip.triplet_finish(*args, k, C))
        bad += [lambda: hip.triplet_finish(*a, *o, 0, C), lambda: hip.triplet_finish(*a, *o, k, 0)]
        _refused(bad, o)


@pytest.mark.parametrize("R_", [1, 100])
@pytest.mark.parametrize("C1", [1, 57])
def test_post_pack_triplets(hip, R_, C1):
    g = K.gen(R_ + C1)
    labels = torch.randint(1, 134, (2 * R_,), generator=g)
    r_dists = torch.rand(R_, C1, generator=g)
    sub, obj = torch.randint(0, 100, (R_,), generator=g), torch.randint(0, 100, (R_,), generator=g)
    ins = [_d(t) for t in (labels, r_dists, sub, obj)]
    n = 4 * R_ + R_ * C1

    def launch():
        rec = _nan(n + 5)
        hip.pack_triplets(*ins, rec, R_, C1)
        return (rec,)
    rec, = _twice(launch)
    assert _is_fence(rec[n:])                    # the fence behind the record
    want = torch.cat([labels.float(), r_dists.reshape(-1), sub.float(), obj.float()])
    assert _same_bits(rec[:n], _d(want))
    if R_ == 1 and C1 == 1:
        bad = []
        for i in range(5):
            args = ins + [rec]
            args[i] = None
            bad.append(lambda args=args: hip.pack_triplets(*args, R_, C1))
        bad += [lambda: hip.pack_triplets(*ins, rec, 0, C1), lambda: hip.pack_triplets(*ins, rec, R_, 0)]
        _refused(bad, [rec])


# ============================================================ pn_panoptic_f32
@pytest.mark.parametrize("n", K.PAN_N)
@pytest.mark.parametrize("HW", K.PAN_HW)
def test_post_panoptic(hip, n, HW):
    masks, labels, remap = K.panoptic_input(n, HW, 0)
    md, ld, rd = _d(masks), _d(labels), _d(remap)
    for rm, rmd in ((None, None), (remap, rd)):
        def launch():
            seg, area = _fi64(HW + 5), _fi32(n + 2)
            area[:n] = 0
            hip.panoptic(md, ld, rmd, seg, area, n, HW)
            return seg, area
        seg, area = _twice(launch)
        assert _fence(seg[HW:]) and _fence(area[n:])
        want_seg, want_area = R.panoptic(masks, labels, rm)
        assert torch.equal(seg[:HW].cpu(), want_seg)         # exact ties: the first index
        assert torch.equal(area[:n].cpu(), want_area) and int(area[:n].sum()) == HW
    if n == 2 and HW == 255:
        _refused([lambda: hip.panoptic(None, ld, None, seg, area, n, HW),
                  lambda: hip.panoptic(md, None, None, seg, area, n, HW),
                  lambda: hip.panoptic(md, ld, None, None, area, n, HW),
                  lambda: hip.panoptic(md, ld, None, seg, None, n, HW),
                  lambda: hip.panoptic(md, ld, None, seg, area, 0, HW),
                  lambda: hip.panoptic(md, ld, None, seg, area, n, 0)], [seg, area])


# ============================================================ the device-side panoptic loop
class _Pan:
    """One scene's device buffers, fenced: the state (behind it 64 bytes of 0xAB), the resized
    planes (one spare plane), the area counters (8 spare words) and seg (5 spare)."""

    def __init__(self, hip, scene):
        self.hip, self.s = hip, scene
        self.Q, self.h, self.w = scene["Q"], scene["h"], scene["w"]
        self.ho, self.wo = scene.get("ho", self.h), scene.get("wo", self.w)
        self.HW = self.ho * self.wo
        self.nb = hip.panoptic_state_bytes()
        self.state = torch.full((self.nb + 64,), 0xAB, device=DEV, dtype=torch.uint8)
        self.up = _nan(self.Q + 1, self.HW)
        self.area = _fi32(256 + 8)
        self.seg = _fi64(self.HW + 5)
        self.masks, self.labels, self.scores = _d(scene["masks"]), _d(scene["labels"]), _d(scene["scores"])
        self.done = 0

    def start(self, rounds):
        self.hip.panoptic_device(self.masks, self.labels, self.scores, self.Q, self.s["NC"], self.h,
                                 self.w, self.ho, self.wo, self.state, self.up, self.area, self.seg,
                                 rounds=rounds)
        self.done = rounds
        return self

    def more(self, rounds):
        self.hip.panoptic_continue(self.state, self.up, self.area, self.seg, self.ho, self.wo,
                                   rounds=rounds)
        self.done += rounds
        return self

    def words(self):
        torch.cuda.synchronize()
        return self.state[:self.nb].view(torch.int32).cpu().numpy()

    def bits(self):
        torch.cuda.synchronize()
        return [self.state.clone(), self.up.clone(), self.seg.clone(), self.area.clone()]

    def check(self, up64=None, seg_exact=True):
        """State words, seg and the fences against the statement after `done` rounds."""
        s = self.s
        if up64 is None:
            up64 = s["masks"].view(self.Q, -1).double().numpy()      # resized 1:1: the source value
        ref = R.panoptic_loop(up64, s["labels"], s["scores"], s["NC"] - 1, self.done)
        w, n = self.words(), ref["nkeep"]
        got = dict(nkeep=int(w[K.ST_NKEEP]), active=int(w[K.ST_ACTIVE]), rounds=int(w[K.ST_ROUNDS]),
                   all_gone=int(w[K.ST_GONE]))
        assert got == {k: ref[k] for k in got}, (got, ref)
        for name, at in (("kept", K.ST_KEPT), ("remap", K.ST_REMAP), ("alive", K.ST_ALIVE),
                         ("rank", K.ST_RANK)):
            assert np.array_equal(w[at:at + n], ref[name]), (name, w[at:at + n], ref[name])
        assert bool((self.state[self.nb:] == 0xAB).all())
        assert _fence(self.seg[self.HW:]) and _fence(self.area[256:]) and _is_fence(self.up[n:])
        assert bool((self.area[:256] == 0).all())                    # cleared for the next round
        if seg_exact:
            assert np.array_equal(self.seg[:self.HW].cpu().numpy(), ref["seg"])
        return ref


@pytest.mark.parametrize("name", ["threshold", "merge", "nkeep0", "all_gone", "single", "ties"])
def test_post_panoptic_device(hip, name):
    scene = K.pan_scenes()[name]
    a = _Pan(hip, scene).start(4)
    ref = a.check()
    assert ref["active"] == 0
    bits_a = a.bits()
    assert all(_eq(x, y) for x, y in zip(bits_a, _Pan(hip, scene).start(4).bits()))   # twice
    # rounds = 1, then one round per continue call: every intermediate state, and the same end
    b = _Pan(hip, scene).start(1)
    b.check()
    for _ in range(3):
        b.more(1).check()
    assert all(_eq(x, y) for x, y in zip(bits_a, b.bits()))
    # a call after convergence changes nothing
    a.more(2)
    assert all(_eq(x, y) for x, y in zip(bits_a, a.bits()))
    if name == "nkeep0":
        assert bool((a.seg[:a.HW] == 1).all())
    if name == "all_gone":
        assert int(a.words()[K.ST_GONE]) == 1


def test_post_panoptic_device_upsampled(hip):
    """7 x 9 -> 13 x 20, random planes: the state words are exact; a pixel's id is admissible
    if its plane's float64 value is within the resize's bound of the winner's, and exact where
    the winner's float64 margin exceeds the bound."""
    scene = K.pan_up_scene()
    Q, ho, wo = scene["Q"], scene["ho"], scene["wo"]
    up64, mag, spread = fwd_ref.bilinear(scene["masks"], ho, wo)
    o32 = F.interpolate(scene["masks"][None], (ho, wo), mode="bilinear", align_corners=False)[0]
    bound, _ = R.value_bound(up64, mag, fwd_cases.BIL_L, None, o32)
    bound = (bound + U * fwd_cases.bilinear_extra(scene["h"], scene["w"], spread)).reshape(Q, -1)
    up64 = up64.reshape(Q, -1)
    p = _Pan(hip, scene).start(4)
    ref = p.check(up64.numpy(), seg_exact=False)
    assert ref["rounds"] == 0
    kept = torch.from_numpy(ref["kept"]).long()
    seg = p.seg[:p.HW].cpu()
    ids = seg // 1000
    assert bool(((ids >= 0) & (ids < len(kept))).all())
    assert torch.equal(seg % 1000, torch.from_numpy(ref["klab"])[ids])
    v, b = up64[kept], bound[kept]
    top, win = v.max(0)
    slack = b.gather(0, ids[None])[0] + b.gather(0, win[None])[0]
    assert bool((top - v.gather(0, ids[None])[0] <= slack).all()), "inadmissible id"
    rest = v.clone()
    rest.scatter_(0, win[None], -math.inf)
    clear = ((top[None] - rest) > (b + b.gather(0, win[None]))).all(0)
    assert float(clear.double().mean()) >= 0.99 and torch.equal(ids[clear], win[clear])


def test_post_panoptic_device_refusals(hip):
    scene = K.pan_scenes()["threshold"]
    p = _Pan(hip, scene)
    m, l, s, Q, NC, h, w = p.masks, p.labels, p.scores, p.Q, scene["NC"], p.h, p.w
    st, up, ar, sg = p.state, p.up, p.area, p.seg

    def dev(*a, **kw):
        return lambda: hip.panoptic_device(*a, **kw)
    calls = [dev(None, l, s, Q, NC, h, w, h, w, st, up, ar, sg), dev(m, None, s, Q, NC, h, w, h, w, st, up, ar, sg),
             dev(m, l, None, Q, NC, h, w, h, w, st, up, ar, sg), dev(m, l, s, Q, NC, h, w, h, w, None, up, ar, sg),
             dev(m, l, s, Q, NC, h, w, h, w, st, None, ar, sg), dev(m, l, s, Q, NC, h, w, h, w, st, up, None, sg),
             dev(m, l, s, Q, NC, h, w, h, w, st, up, ar, None),
             dev(m, l, s, 0, NC, h, w, h, w, st, up, ar, sg), dev(m, l, s, 257, NC, h, w, h, w, st, up, ar, sg),
             dev(m, l, s, Q, NC, h, w, h, w, st, up, ar, sg, rounds=0),
             dev(m, l, s, Q, NC, h, w, h, w, st, up, ar, sg, rounds=257),
             dev(m, l, s, Q, NC, 0, w, h, w, st, up, ar, sg), dev(m, l, s, Q, NC, h, 0, h, w, st, up, ar, sg),
             dev(m, l, s, Q, NC, h, w, 0, w, st, up, ar, sg), dev(m, l, s, Q, NC, h, w, h, 0, st, up, ar, sg),
             dev(m, l, s, Q, NC, h, w, h, (1 << 24) + 1, st, up, ar, sg),
             lambda: hip.panoptic_continue(None, up, ar, sg, h, w), lambda: hip.panoptic_continue(st, None, ar, sg, h, w),
             lambda: hip.panoptic_continue(st, up, None, sg, h, w), lambda: hip.panoptic_continue(st, up, ar, None, h, w),
             lambda: hip.panoptic_continue(st, up, ar, sg, 0, w), lambda: hip.panoptic_continue(st, up, ar, sg, h, 0),
             lambda: hip.panoptic_continue(st, up, ar, sg, h, w, rounds=0),
             lambda: hip.panoptic_continue(st, up, ar, sg, h, w, rounds=257),
             lambda: hip.resize_kept(None, up, st, Q, h, w, h, w), lambda: hip.resize_kept(m, None, st, Q, h, w, h, w),
             lambda: hip.resize_kept(m, up, None, Q, h, w, h, w), lambda: hip.resize_kept(m, up, st, 0, h, w, h, w),
             lambda: hip.resize_kept(m, up, st, 257, h, w, h, w), lambda: hip.resize_kept(m, up, st, Q, 0, w, h, w),
             lambda: hip.resize_kept(m, up, st, Q, h, 0, h, w), lambda: hip.resize_kept(m, up, st, Q, h, w, 0, w),
             lambda: hip.resize_kept(m, up, st, Q, h, w, h, 0),
             lambda: hip.resize_kept(m, up, st, Q, h, w, h, (1 << 24) + 1),
             lambda: hip.resize_kept(m, up, st, Q, h, w, h, w, form=-1),
             lambda: hip.resize_kept(m, up, st, Q, h, w, h, w, form=2)]
    _refused(calls, [st, up, ar, sg])


# ============================================================ pn_resize_kept_f32
@pytest.mark.parametrize("nkeep", K.RESIZE_NKEEP)
@pytest.mark.parametrize("shape", K.RESIZE_SHAPES, ids=lambda s: "%dx%d_%dx%d" % s)
def test_post_resize_kept(hip, nkeep, shape):
    """L = 5 (fwd_cases.BIL_L) with the coordinate term of the planar resize; both forms, bit-equal
    to each other and to pn_bilinear_planar_f32 on the gathered planes."""
    hi, wi, ho, wo = shape
    Q = 10
    g = K.gen(nkeep + wo)
    mp = torch.randn(Q, hi, wi, generator=g) * 4.0
    kept = torch.randperm(Q, generator=g)[:nkeep]
    state = torch.zeros(hip.panoptic_state_bytes() // 4, dtype=torch.int32)
    state[K.ST_NKEEP] = nkeep
    state[K.ST_KEPT:K.ST_KEPT + nkeep] = kept.to(torch.int32)
    state, mpd = _d(state).view(torch.uint8), _d(mp)
    ups = []
    for form in (0, 1):
        def launch():
            up = _nan(Q + 1, ho * wo)
            hip.resize_kept(mpd, up, state, Q, hi, wi, ho, wo, form=form)
            return (up,)
        ups.append(_twice(launch)[0])
    assert _same_bits(ups[0], ups[1])
    assert _is_fence(ups[0][nkeep:])              # planes from nkeep on
    if nkeep == 0:
        return
    planar = _nan(nkeep * ho * wo + 4)
    hip.bilinear_planar(_d(mp[kept].contiguous()), planar, nkeep, hi, wi, ho, wo)
    torch.cuda.synchronize()
    assert _same_bits(ups[0][:nkeep].reshape(-1), planar[:nkeep * ho * wo])
    ref, mag, spread = fwd_ref.bilinear(mp[kept], ho, wo)
    o32 = F.interpolate(mp[kept][None], (ho, wo), mode="bilinear", align_corners=False)[0]
    _bounded("k_resize_kept", "%dx%d -> %dx%d nkeep %d" % (hi, wi, ho, wo, nkeep),
             ups[0][:nkeep].view(nkeep, ho, wo), ref, mag, fwd_cases.BIL_L, o32,
             extra=fwd_cases.bilinear_extra(hi, wi, spread))


# ============================================================ top-k
def _topk_check(idx, quot, rem, x, k, div, B):
    assert _fence(idx[B * k:]) and _fence(quot[B * k:]) and _fence(rem[B * k:])
    want = R.topk(x.numpy(), k)
    got = idx[:B * k].view(B, k).cpu()
    assert torch.equal(got, want), (x.shape, k, (got != want).nonzero()[:4])
    assert torch.equal(quot[:B * k].view(B, k).cpu(), want // div)
    assert torch.equal(rem[:B * k].view(B, k).cpu(), want % div)


@pytest.mark.parametrize("n", K.TOPK_N)
def test_post_topk(hip, n):
    B, div = 3, 57
    for k in K.topk_ks(n):
        for seed in (0, 3, 6):                    # all nine kinds of row
            x = K.topk_input(n, k, B, seed)
            xd = _d(x)

            def launch():
                outs = _fi64(B * k + 4), _fi64(B * k + 4), _fi64(B * k + 4)
                hip.topk(xd, *outs, B, n, div, k)
                return outs
            _topk_check(*_twice(launch), x, k, div, B)


@pytest.mark.parametrize("es", [1, 3, 91])
@pytest.mark.parametrize("n", K.TOPK_N)
def test_post_topk_strided(hip, n, es):
    """Every skipped element and the gap between rows hold NaN."""
    B, div = 3, 91
    rs = n * es + 7
    for j, k in enumerate(K.topk_ks(n, strided=True)):
        for seed in ((0, 3, 6) if es == 1 else ((3 * j) % 9,)):
            x = K.topk_input(n, k, B, seed)
            buf = _nan(B * rs + 3)
            buf[:B * rs].view(B, rs)[:, :n * es:es] = _d(x)

            def launch():
                outs = _fi64(B * k + 4), _fi64(B * k + 4), _fi64(B * k + 4)
                hip.topk_strided(buf, es, rs, *outs, B, n, div, k)
                return outs
            _topk_check(*_twice(launch), x, k, div, B)


@pytest.mark.parametrize("Q", K.TOPK_Q)
def test_post_topk_pairs(hip, Q):
    B, n = 3, Q * Q
    for k in K.topk_ks(n):
        for seed in (0, 3, 6):
            x = K.topk_input(n, k, B, seed)
            xd = _d(x)
            for with_pair in (False, True):
                def launch():
                    outs = [_fi64(B * k + 4), _fi64(B * k + 4), _fi64(B * k + 4), _fi64(B * 2 * k + 4)]
                    hip.topk_pairs(xd, outs[0], outs[1], outs[2], B, Q, k,
                                   pair=outs[3] if with_pair else None)
                    return outs
                idx, sub, obj, pair = _twice(launch)
                _topk_check(idx, sub, obj, x, k, Q, B)
                if with_pair:
                    want = R.topk(x.numpy(), k)
                    assert _fence(pair[B * 2 * k:])
                    assert torch.equal(pair[:B * 2 * k].view(B, 2 * k).cpu(),
                                       torch.cat([want // Q, want % Q], 1))
                else:
                    assert _fence(pair)


def test_post_topk_refusals(hip):
    x = _d(torch.randn(3, 100, generator=K.gen(0)))
    i, q, r, p = _fi64(64), _fi64(64), _fi64(64), _fi64(64)
    big = _d(torch.zeros(1))
    _refused([
        lambda: hip.topk_pairs(None, i, q, r, 1, 10, 5), lambda: hip.topk_pairs(x, None, q, r, 1, 10, 5),
        lambda: hip.topk_pairs(x, i, None, r, 1, 10, 5), lambda: hip.topk_pairs(x, i, q, None, 1, 10, 5),
        lambda: hip.topk_pairs(x, i, q, r, 0, 10, 5), lambda: hip.topk_pairs(x, i, q, r, 1, 0, 5),
        lambda: hip.topk_pairs(big, i, q, r, 1, 257, 5), lambda: hip.topk_pairs(x, i, q, r, 1, 10, 0),
        lambda: hip.topk_pairs(x, i, q, r, 1, 10, 257), lambda: hip.topk_pairs(x, i, q, r, 1, 2, 5),
        lambda: hip.topk(None, i, q, r, 1, 100, 7, 5), lambda: hip.topk(x, None, q, r, 1, 100, 7, 5),
        lambda: hip.topk(x, i, None, r, 1, 100, 7, 5), lambda: hip.topk(x, i, q, None, 1, 100, 7, 5),
        lambda: hip.topk(x, i, q, r, 0, 100, 7, 5), lambda: hip.topk(x, i, q, r, 1, 0, 7, 5),
        lambda: hip.topk(x, i, q, r, 1, 100, 0, 5), lambda: hip.topk(big, i, q, r, 1, 65537, 7, 5),
        lambda: hip.topk(x, i, q, r, 1, 100, 7, 0), lambda: hip.topk(x, i, q, r, 1, 300, 7, 257),
        lambda: hip.topk(x, i, q, r, 1, 5, 7, 6),
        lambda: hip.topk_strided(None, 1, 100, i, q, r, 1, 100, 7, 5),
        lambda: hip.topk_strided(x, 1, 100, None, q, r, 1, 100, 7, 5),
        lambda: hip.topk_strided(x, 1, 100, i, None, r, 1, 100, 7, 5),
        lambda: hip.topk_strided(x, 1, 100, i, q, None, 1, 100, 7, 5),
        lambda: hip.topk_strided(x, 1, 100, i, q, r, 0, 100, 7, 5),
        lambda: hip.topk_strided(x, 1, 100, i, q, r, 1, 0, 7, 5),
        lambda: hip.topk_strided(x, 1, 100, i, q, r, 1, 100, 0, 5),
        lambda: hip.topk_strided(x, 0, 100, i, q, r, 1, 100, 7, 5),
        lambda: hip.topk_strided(big, 1, 100, i, q, r, 1, 65537, 7, 5),
        lambda: hip.topk_strided(x, 1, 100, i, q, r, 1, 100, 7, 0),
        lambda: hip.topk_strided(big, 1, 600, i, q, r, 1, 600, 7, 513),
        lambda: hip.topk_strided(x, 1, 100, i, q, r, 1, 5, 7, 6),
    ], [i, q, r, p])


# ============================================================ pn_zero_rows_f32
@pytest.mark.parametrize("C", [4, 256])
@pytest.mark.parametrize("rows", [1, 50, 257])
def test_post_zero_rows(hip, C, rows):
    """out = where(valid, x, +0): invalid rows hold NaN, +-inf and -0 and must come out +0; the
    columns from C to ld keep their bits."""
    for B in (1, 2):
        for ld in (C, C + 8):
            for per_image in (False, True):
                x, valid = K.zero_rows_input(B, rows, C, ld, B + ld, per_image)
                want = _d(R.zero_rows(x[..., :C], valid.expand(B, rows)))
                xd, vd = _d(x), _d(valid.to(torch.uint8).contiguous())

                def out_of_place():
                    out = _nan(B * rows * ld + 8)
                    hip.zero_rows(xd, vd, out, B, rows, C, ld=ld, per_image=per_image)
                    return (out,)
                out, = _twice(out_of_place)
                assert _is_fence(out[B * rows * ld:])
                out = out[:B * rows * ld].view(B, rows, ld)
                assert _same_bits(out[..., :C], want) and _is_fence(out[..., C:])

                def in_place():
                    buf = xd.clone()
                    hip.zero_rows(buf, vd, buf, B, rows, C, ld=ld, per_image=per_image)
                    return (buf,)
                buf, = _twice(in_place)
                assert _same_bits(buf[..., :C], want) and _same_bits(buf[..., C:], xd[..., C:])
    if C == 4 and rows == 50:
        o = _nan(B * rows * ld + 8)
        z = lambda *a, **kw: (lambda: hip.zero_rows(*a, **kw))
        _refused([z(None, vd, o, B, rows, C, ld=ld), z(xd, None, o, B, rows, C, ld=ld),
                  z(xd, vd, None, B, rows, C, ld=ld), z(xd, vd, o, 0, rows, C, ld=ld),
                  z(xd, vd, o, B, 0, C, ld=ld), z(xd, vd, o, B, rows, 0, ld=ld),
                  z(xd, vd, o, B, rows, 6, ld=ld), z(xd, vd, o, B, rows, 8, ld=4),
                  z(xd, vd, o, B, rows, C, ld=C + 2), z(xd.view(-1)[1:], vd, o, B, rows, C, ld=ld),
                  z(xd, vd, o.view(-1)[1:], B, rows, C, ld=ld)], [o])
        lib = hip.lib()
        assert lib.pn_zero_rows_f32(xd.data_ptr(), vd.data_ptr(), o.data_ptr(), B, rows, C, ld, -1,
                                    None) == -1
        torch.cuda.synchronize()
        assert _is_fence(o)


# ============================================================ box embedding, refinement
# k_box_pos_embed.  ref: L = 4 (exp 2, the sum, the quotient).  emb: L = 4 (sin / cos at 2 ulp),
# cond = 9 |argument| (post_ref.POS_ARG_L), mag = 1.
@pytest.mark.parametrize("rows", [1, 3, 300])
def test_post_box_pos_embed(hip, rows):
    from oracle.deformable_detr import DeformableDetrTransformer as T
    x = K.box_logits(rows, 0)
    xd = _d(x)

    def launch():
        ref, emb = _nan(rows * 4 + 4), _nan(rows * 512 + 8)
        hip.box_pos_embed(xd, ref, emb, rows)
        return ref, emb
    ref, emb = _twice(launch)
    assert _is_fence(ref[rows * 4:]) and _is_fence(emb[rows * 512:])
    s, e, emag, econd = R.box_pos_embed(x)
    case = "rows %d" % rows
    _bounded("k_box_pos_embed:ref", case, ref[:rows * 4].view(rows, 4), s, s, 4, x.sigmoid())
    _bounded("k_box_pos_embed:emb", case, emb[:rows * 512].view(rows, 512), e, emag, 4,
             T.get_proposal_pos_embed(x[None])[0], cond=econd)
    if rows == 1:
        _refused([lambda: hip.box_pos_embed(None, ref, emb, 1), lambda: hip.box_pos_embed(xd, None, emb, 1),
                  lambda: hip.box_pos_embed(xd, ref, None, 1), lambda: hip.box_pos_embed(xd, ref, emb, 0)],
                 [ref, emb])


# k_box_refine.  L = 4 (the last sigmoid: exp 2, the sum, the quotient); cond = 3 + 2 |log q| +
# |z| (post_ref.box_refine): near 0 and 1 the logarithm's own rounding dominates.
@pytest.mark.parametrize("rows", [1, 64, 65])
def test_post_box_refine(hip, rows):
    from oracle.deformable_detr import inverse_sigmoid
    delta, ref_in = K.refine_input(rows, rows)
    dd, rd = _d(delta), _d(ref_in)

    def launch():
        out = _nan(rows * 4 + 4)
        hip.box_refine(dd, rd, out, rows)
        return (out,)
    out, = _twice(launch)
    assert _is_fence(out[rows * 4:])
    ref, mag, cond = R.box_refine(delta, ref_in)
    _bounded("k_box_refine", "rows %d" % rows, out[:rows * 4].view(rows, 4), ref, mag, 4,
             (delta + inverse_sigmoid(ref_in)).sigmoid(), cond=cond)
    if rows == 1:
        _refused([lambda: hip.box_refine(None, rd, out, 1), lambda: hip.box_refine(dd, None, out, 1),
                  lambda: hip.box_refine(dd, rd, None, 1), lambda: hip.box_refine(dd, rd, out, 0)], [out])


# ============================================================ sampling operands
# weights: L = NP + 4 (exp 2 on either side, NP - 1 sequential adds, the quotient), cond of the
# softmax.  box locations: L = 4 (c r, wh r, the product with offset / 4, the sum; / 4 and * 0.5
# are exact).  token locations: L = 5 (vr W, the quotient, x vr, offset / W, the sum).
def _o32_aw(offaw, NP):
    lead = offaw.shape[:-1]
    return F.softmax(offaw[..., 8 * NP * 2:8 * NP * 3].reshape(*lead, 8, NP), -1)


@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("B,rpi", [(3, 5), (2, 35)])
def test_post_box_sampling(hip, L, B, rpi):
    rows, NP = B * rpi, L * 4
    for ld_extra in (0, 4):
        offaw, ref, vr = K.box_sampling_input(B, rpi, L, ld_extra, ld_extra)
        ld = offaw.shape[1]
        od, rd, vd = _d(offaw), _d(ref), _d(vr)
        for ratios, rdv in ((None, None), (vr, vd)):
            def launch():
                loc, aw = _nan(rows * 8 * NP * 2 + 4), _nan(rows * 8 * NP + 4)
                hip.box_sampling(od, ld, rd, loc, aw, rows, L, valid_ratios=rdv,
                                 rows_per_image=rpi if ratios is not None else 0)
                return loc, aw
            loc, aw = _twice(launch)
            assert _is_fence(loc[rows * 8 * NP * 2:]) and _is_fence(aw[rows * 8 * NP:])
            rl, lmag, ra, amag, acond = R.box_sampling(offaw, ref, L, ratios, rpi)
            # torch's fp32 evaluation of the same formulas
            off = offaw[:, :8 * NP * 2].view(rows, 8, NP, 2)
            r = torch.ones(rows, L, 2) if ratios is None else ratios[torch.arange(rows) // rpi]
            r = r.repeat_interleave(4, 1)[:, None]
            o32 = ref[:, None, None, :2] * r + off / 4 * (ref[:, None, None, 2:] * r) * 0.5
            case = "L %d rows %d ld +%d %s" % (L, rows, ld_extra, "ratios" if ratios is not None else "plain")
            _bounded("k_box_sampling:loc", case, loc[:rows * 8 * NP * 2].view(rows, 8, NP, 2), rl,
                     lmag, 4, o32)
            _bounded("k_box_sampling:aw", case, aw[:rows * 8 * NP].view(rows, 8, NP), ra, amag,
                     NP + 4, _o32_aw(offaw, NP), cond=acond)
    if L == 2 and B == 3:
        b = lambda *a, **kw: (lambda: hip.box_sampling(*a, **kw))
        _refused([b(None, ld, rd, loc, aw, rows, L), b(od, ld, None, loc, aw, rows, L),
                  b(od, ld, rd, None, aw, rows, L), b(od, ld, rd, loc, None, rows, L),
                  b(od, ld, rd, loc, aw, 0, L), b(od, ld, rd, loc, aw, rows, 0),
                  b(od, ld, rd, loc, aw, rows, 5), b(od, 8 * L * 12 - 1, rd, loc, aw, rows, L),
                  b(od, ld, rd, loc, aw, rows, L, valid_ratios=vd, rows_per_image=0)], [loc, aw])


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_post_token_sampling(hip, L):
    B, NP = 2, L * 4
    for ld_extra in (0, 4):
        offaw, vr, shapes = K.token_sampling_input(L, B, ld_extra, ld_extra)
        N, ld = offaw.shape[1], offaw.shape[2]
        od, vd = _d(offaw), _d(vr)

        def launch():
            loc, aw = _nan(B * N * 8 * NP * 2 + 4), _nan(B * N * 8 * NP + 4)
            hip.token_sampling(od, ld, vd, loc, aw, B, shapes)
            return loc, aw
        loc, aw = _twice(launch)
        assert _is_fence(loc[B * N * 8 * NP * 2:]) and _is_fence(aw[B * N * 8 * NP:])
        loc, aw = loc[:B * N * 8 * NP * 2].view(B, N, 8, NP, 2), aw[:B * N * 8 * NP].view(B, N, 8, NP)
        rl, lmag, ra, amag, acond = R.token_sampling(offaw, vr, shapes)
        from oracle.deformable_detr import DeformableDetrTransformer as T
        wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32)
        o32 = T.get_reference_points(shapes, vr)[:, :, None, :, None, :] + \
            offaw[..., :8 * NP * 2].view(B, N, 8, L, 4, 2) / wh[None, None, None, :, None, :]
        o32 = o32.reshape(B, N, 8, NP, 2)
        case = "L %d ld +%d" % (L, ld_extra)
        _bounded("k_token_sampling:loc", case, loc, rl, lmag, 5, o32)
        _bounded("k_token_sampling:aw", case, aw, ra, amag, NP + 4, _o32_aw(offaw, NP), cond=acond)
        for n in K.level_edges(shapes):          # the first and the last token of every level
            _bounded("k_token_sampling:loc", case + " token %d" % n, loc[:, n], rl[:, n], lmag[:, n],
                     5, o32[:, n])
    t = lambda *a: (lambda: hip.token_sampling(*a))
    _refused([t(None, ld, vd, loc, aw, B, shapes), t(od, ld, None, loc, aw, B, shapes),
              t(od, ld, vd, None, aw, B, shapes), t(od, ld, vd, loc, None, B, shapes),
              t(od, ld, vd, loc, aw, 0, shapes), t(od, ld, vd, loc, aw, B, []),
              t(od, ld, vd, loc, aw, B, shapes + [(1, 1)] * (5 - L)),
              t(od, 8 * L * 12 - 1, vd, loc, aw, B, shapes),
              t(od, ld, vd, loc, aw, B, [(0, 3)] + shapes[1:]),
              t(od, ld, vd, loc, aw, B, shapes[:-1] + [(2, 0)])], [loc, aw])


# ============================================================ pn_query_score_f32
# L = Nq + 4: exp (2) on either side, Nq - 1 sequential adds over the queries, the quotient; the
# maximum over the classes rounds nothing.  cond: the largest of the query's (q, c) terms.
@pytest.mark.parametrize("C", K.QS_C)
def test_post_query_score(hip, C):
    for B in K.QS_B:
        for Nq in K.QS_NQ:
            x = K.query_score_input(B, Nq, C, B)
            xd = _d(x)

            def launch():
                score = _nan(B * Nq + 3)
                hip.query_score(xd, score, B, Nq, C)
                return (score,)
            score, = _twice(launch)
            assert _is_fence(score[B * Nq:])
            ref, mag, cond = R.query_score(x)
            _bounded("k_query_score", "B %d Nq %d C %d" % (B, Nq, C), score[:B * Nq].view(B, Nq),
                     ref, mag, Nq + 4, F.softmax(x, dim=1).max(-1)[0], cond=cond)
    if C == 1:
        q = lambda *a: (lambda: hip.query_score(*a))
        _refused([q(None, score, B, Nq, C), q(xd, None, B, Nq, C), q(xd, score, 0, Nq, C),
                  q(xd, score, B, 0, C), q(xd, score, B, Nq, 0), q(xd, score, B, Nq, 257)], [score])


# ============================================================ pn_box_triplets_f32
# score: L = 9 + ceil(C / 64) (exp 2, ceil(C / 64) in-lane adds, 6 shuffle adds, the quotient),
# cond = sum p |d|.  box: L = 3 (centre -+ half, x image size, / scale factor; the clamp is exact).
@pytest.mark.parametrize("R_", K.TRIP_R)
@pytest.mark.parametrize("C", K.TRIP_C)
def test_post_box_triplets(hip, R_, C):
    import types
    from oracle.bbox_head import OracleCrossHeadBBox as H
    ins = K.box_triplets_input(R_, C, R_)
    ind = [_d(t) for t in ins]
    img_h, img_w = 48.0, 80.0                     # not square
    me = types.SimpleNamespace(num_relations=2, num_rel_query=1)
    for rescale in (False, True):
        def launch():
            det, labels = _nan(2 * R_ * 5 + 5), _fi64(2 * R_ + 3)
            hip.box_triplets(*ind, det, labels, R_, C, img_h, img_w, K.TRIP_SF, rescale)
            return det, labels
        det, labels = _twice(launch)
        assert _is_fence(det[2 * R_ * 5:]) and _fence(labels[2 * R_:])      # behind row 2R
        want, ref, mag, cond = R.box_triplets(*ins, img_h, img_w, K.TRIP_SF, rescale)
        assert torch.equal(labels[:2 * R_].cpu(), want), (labels[:2 * R_].cpu(), want)
        o32 = H._get_bboxes_single(me, ins[0], ins[1], torch.zeros(1, 2), ins[2], ins[3],
                                   (48, 80, 3), K.TRIP_SF, rescale)[0]
        Lc = torch.tensor([3.0, 3.0, 3.0, 3.0, 9.0 + -(-C // 64)]).expand(2 * R_, 5)
        cd = torch.cat([torch.zeros(2 * R_, 4, dtype=torch.float64), cond[:, None]], 1)
        _bounded("k_box_triplets", "R %d C %d rescale %d" % (R_, C, rescale),
                 det[:2 * R_ * 5].view(2 * R_, 5), ref, mag, Lc, o32, cond=cd)
    if R_ == 1 and C == 2:
        bad = []
        for i in range(6):
            args = ind + [det, labels]
            args[i] = None
            bad.append(lambda args=args: hip.box_triplets(*args, R_, C, img_h, img_w, K.TRIP_SF, True))
        bad += [lambda: hip.box_triplets(*ind, det, labels, 0, C, img_h, img_w, K.TRIP_SF, True),
                lambda: hip.box_triplets(*ind, det, labels, R_, 0, img_h, img_w, K.TRIP_SF, True)]
        _refused(bad, [det, labels])
        lib = hip.lib()                           # rescale without scale factors
        assert lib.pn_box_triplets_f32(*[t.data_ptr() for t in ind], det.data_ptr(),
                                       labels.data_ptr(), R_, C, img_h, img_w, None, 1, None) == -1


# ============================================================ pn_sine_pe_valid_f32
# L = 5 (sin / cos at 2 ulp, the added vector), mag = 1 + |add|, cond = |argument| x its rounding
# count (post_ref.sine_pe).  Where the normaliser is zero and the offset is not, the argument is
# about 3e6 and no bound means anything: there only "finite, and |out - add| <= 1" is asserted
# (with `add`, up to the one rounding of that sum: 2^-24 (1 + |add|)).
@pytest.mark.parametrize("h,w", K.SINE_HW)
@pytest.mark.parametrize("C", K.SINE_C)
def test_post_sine_pe(hip, h, w, C):
    from oracle.layers import SinePositionalEncoding
    g = K.gen(h + C)
    for vh, vw in K.sine_valids(h, w):
        for offset in (0.0, -0.5):
            for T in (10000.0, 20.0):
                for add in (None, torch.randn(C, generator=g)):
                    addd = None if add is None else _d(add)

                    def launch():
                        out = _nan(h * w * C + 8)
                        hip.sine_pe(out, addd, h, w, C_=C, temperature=T, offset=offset, valid=(vh, vw))
                        return (out,)
                    out, = _twice(launch)
                    assert _is_fence(out[h * w * C:])
                    out = out[:h * w * C].view(h * w, C).cpu()
                    ref, mag, cond, wild = R.sine_pe(h, w, C, vh, vw, T, offset, add)
                    mask = torch.ones(1, h, w, dtype=torch.bool)
                    mask[:, :vh, :vw] = False
                    o32 = SinePositionalEncoding(C // 2, temperature=T, normalize=True,
                                                 offset=offset)(mask)[0].permute(1, 2, 0).reshape(h * w, C)
                    if add is not None:
                        o32 = o32 + add
                    if bool(wild.any()):
                        a64 = torch.zeros(C, dtype=torch.float64) if add is None else add.double()
                        lim = (1.0 + (U * (1.0 + a64.abs()) if add is not None else a64)).expand(h * w, C)
                        assert bool(torch.isfinite(out[wild]).all())
                        assert bool(((out.double() - a64).abs() <= lim)[wild].all())
                    ok = ~wild
                    _bounded("k_sine_pe", "%dx%d C %d valid %dx%d off %g T %g%s" % (
                        h, w, C, vh, vw, offset, T, " +add" if add is not None else ""),
                        _d(out[ok]), ref[ok], mag[ok], 5, o32[ok], cond=cond[ok])
    if C == 4:
        s = lambda *a, **kw: (lambda: hip.sine_pe(*a, **kw))
        o = _nan(h * w * C + 8)
        _refused([s(None, None, h, w, C_=C), s(o, None, 0, w, C_=C), s(o, None, h, 0, C_=C),
                  s(o, None, h, w, C_=0), s(o, None, h, w, C_=6), s(o, None, h, w, C_=C, valid=(0, w)),
                  s(o, None, h, w, C_=C, valid=(h + 1, w)), s(o, None, h, w, C_=C, valid=(h, 0)),
                  s(o, None, h, w, C_=C, valid=(h, w + 1))], [o])
