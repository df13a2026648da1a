"""GPU: `pn_mha_bwd_keysplit_f32` (csrc/attn_grad.hip), the unmasked attention backward with the keys
split across workgroups, against float64 autograd (`test_grad_kernels_gpu._mha_ref`) under that
file's softmax-type row bound with the project's own constant C_MHA = 115 (not retuned to this
kernel).  Every case also runs `pn_mha_bwd_f32` on the same inputs, prints both worst ratios and
checks that the two kernels differ by at most the sum of their two bounds; two launches of the new
kernel agree bit for bit.  Shapes around the key chunk c = hip.MHA_KEYSPLIT_CHUNK, more queries than
one query tile, and once the finest memory level of an 800 x 1333 image."""
import pytest
import torch

from pairnet_amd.hip import MHA_KEYSPLIT_CHUNK as c
from test_grad_kernels_gpu import (C_MHA, DEV, FLT_MIN, U, _gen, _mha_ref, _randn, _within_rows,
                                   hip)  # noqa: F401  (`hip`: that module's fixture)

pytestmark = pytest.mark.gpu
SCALE = 32 ** -0.5
NAN_BITS = 0x7fc00000

CASES = [(1, 1, 1), (2, 9, 33), (2, 13, 70), (1, 100, c - 1), (1, 100, c), (1, 100, c + 1),
         (2, 37, 3 * c + 5), (1, 130, 2 * c), (1, 100, 16700)]


def _ratio(got, ref):
    """Worst |got - ref| / (2^-24 max |ref row|) beyond FLT_MIN, without asserting."""
    ref = ref.to(DEV).double()
    err = (got.double() - ref).abs()
    mag = ref.abs().amax(-1, keepdim=True).expand_as(ref)
    r = torch.where(err <= FLT_MIN, torch.zeros_like(err), (err - FLT_MIN).clamp_min(0) / (U * mag))
    return float(r.max())


def _keysplit(hip, q, k, v, do, B, Nq, Nk, outs=None):
    dq, dk, dv = outs if outs is not None else \
        (torch.full((B * n, 256), float("nan"), device=DEV) for n in (Nq, Nk, Nk))
    scr = torch.empty(hip.mha_bwd_keysplit_scratch_floats(B, Nq, Nk), device=DEV)
    hip.mha_bwd_keysplit(q, k, v, do, dq, dk, dv, scr, B, Nq, Nk, SCALE)
    return dq, dk, dv


def _parent(hip, q, k, v, do, B, Nq, Nk):
    dq, dk, dv = (torch.full((B * n, 256), float("nan"), device=DEV) for n in (Nq, Nk, Nk))
    scr = torch.empty(hip.mha_bwd_scratch_floats(B, Nq, Nk), device=DEV)
    hip.mha_bwd(q, k, v, do, dq, dk, dv, scr, B, Nq, Nk, SCALE)
    return dq, dk, dv


def _check_case(hip, tag, q, k, v, do, B, Nq, Nk, agree=("dq", "dk", "dv")):
    """`agree`: the outputs on which the two kernels must lie within the sum of their two bounds --
    all three, unless pn_mha_bwd_f32 itself is outside its bound on the input (see the peaked case)."""
    got, got2 = _keysplit(hip, q, k, v, do, B, Nq, Nk), _keysplit(hip, q, k, v, do, B, Nq, Nk)
    par = _parent(hip, q, k, v, do, B, Nq, Nk)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, got2)), "two launches differ"
    refs = _mha_ref(q, k, v, do, B, Nq, Nk, SCALE, None)
    for nm, a, p, r in zip(("dq", "dk", "dv"), got, par, refs):     # every figure before any assertion
        print("%s %s: keysplit worst ratio %.3f, pn_mha_bwd_f32 worst ratio %.3f"
              % (tag, nm, _ratio(a, r), _ratio(p, r)))
    for nm, a, p, r in zip(("dq", "dk", "dv"), got, par, refs):
        _within_rows("%s keysplit %s" % (tag, nm), a, r, C_MHA)
        if nm not in agree:
            continue
        # kernel agreement: at most the sum of the two bounds
        r64 = r.to(DEV).double()
        bound = 2 * (C_MHA * U * r64.abs().amax(-1, keepdim=True) + FLT_MIN)
        assert bool(((a.double() - p.double()).abs() <= bound).all()), "%s %s: kernels disagree" % (tag, nm)
    return got, refs


def test_chunk_constant_is_the_librarys(hip):
    assert hip.lib().pn_mha_keysplit_chunk() == hip.MHA_KEYSPLIT_CHUNK == c
    for B, Nq, Nk in ((1, 1, 1), (2, 37, 3 * c + 5), (1, 100, 16700)):
        want = B * 8 * Nq * (6 + 32 * ((Nk + c - 1) // c))
        assert hip.mha_bwd_keysplit_scratch_floats(B, Nq, Nk) == want
        assert hip.lib().pn_mha_bwd_keysplit_scratch_floats(B, Nq, Nk) == want


@pytest.mark.parametrize("B,Nq,Nk", CASES)
def test_keysplit_against_float64_and_the_parent_kernel(hip, B, Nq, Nk):
    g = _gen(B * 100000 + Nq * 1000 + Nk)
    q, k, v = _randn(g, B * Nq, 256), _randn(g, B * Nk, 256), _randn(g, B * Nk, 256)
    do = _randn(g, B * Nq, 256)
    _check_case(hip, "B%d Nq%d Nk%d" % (B, Nq, Nk), q, k, v, do, B, Nq, Nk)


def test_peaked_softmax(hip):
    """q scaled by 8 (logits of standard deviation 8: most probabilities fall below 2^-24 of their
    row's largest); dq, dk and dv stay finite and inside the bound.

    Measured on the MI355X, worst |err| / (2^-24 max |ref row|), bound 115: dq 6.5, dk 7.6, dv 7.3;
    pn_mha_bwd_f32 on the same inputs: 54.4, 654.0, 95.3.  The existing kernel is outside its own
    bound on dk here (fp32 logits and an fp32 dP - delta, labnotes R23.2; it is not changed by this
    file's subject and no existing test feeds it such an input), so "the two kernels differ by at
    most the sum of their two bounds" cannot hold for dk on this input whatever the new kernel
    does: the agreement is asserted on dq and dv, where it does, and dk is held against float64
    alone."""
    B, Nq, Nk = 2, 37, 3 * c + 5
    g = _gen(88)
    q, k, v = _randn(g, B * Nq, 256, scale=8.0), _randn(g, B * Nk, 256), _randn(g, B * Nk, 256)
    do = _randn(g, B * Nq, 256)
    got, _ = _check_case(hip, "peaked", q, k, v, do, B, Nq, Nk, agree=("dq", "dv"))
    assert all(bool(torch.isfinite(t).all()) for t in got)
    hd = q.double().view(B, Nq, 8, 32).transpose(1, 2) @ \
        k.double().view(B, Nk, 8, 32).transpose(1, 2).transpose(-1, -2)
    P = torch.softmax(SCALE * hd, -1)
    assert float((P < U * P.amax(-1, keepdim=True)).double().mean()) > 0.5, "the case is not peaked"


def test_equal_keys(hip):
    """All keys equal (the memory rows the reference feeds as key AND value: k rows equal, v rows
    equal).  The probabilities are uniform (Nk a power of two: exactly 1 / Nk), dP equals the row
    term, so dS, dq and dk are exactly zero, and every dv row is the mean over the keys of the dO
    column sums.  v and dO are small integers so that fp32 and float64 are both exact."""
    B, Nq, Nk = 1, 100, 2 * c
    assert Nk & (Nk - 1) == 0
    g = _gen(5)
    q = _randn(g, B * Nq, 256)
    k = _randn(g, 1, 256).expand(B * Nk, 256).contiguous()
    v = torch.randint(-3, 4, (1, 256), generator=g, device=DEV).float().expand(B * Nk, 256).contiguous()
    do = torch.randint(-3, 4, (B * Nq, 256), generator=g, device=DEV).float()
    got, refs = _check_case(hip, "equal keys", q, k, v, do, B, Nq, Nk)
    assert int(torch.count_nonzero(got[1])) == 0 and int(torch.count_nonzero(got[0])) == 0
    want = (do.double().sum(0, keepdim=True) / Nk).expand(B * Nk, 256)
    assert torch.equal(got[2].double(), want)


def _fenced(rows, ld, fence=64):
    """A NaN-filled [rows, ld] view of a flat buffer with `fence` more NaN floats behind it."""
    flat = torch.full((rows * ld + fence,), float("nan"), device=DEV)
    return flat, flat[:rows * ld].view(rows, ld)


def test_strided_operands_and_untouched_neighbours(hip):
    """q / dq are column blocks of 768-wide rows, k / v and dk / dv column blocks of 512-wide rows;
    NaNs pre-written in the outputs, their foreign columns and a fence behind each buffer."""
    B, Nq, Nk = 2, 37, 3 * c + 5
    g = _gen(512768)
    QKV, KV = _randn(g, B * Nq, 768), _randn(g, B * Nk, 512)
    do = _randn(g, B * Nq, 256)
    q, k, v = QKV[:, 256:512], KV[:, :256], KV[:, 256:]
    fq, dQKV = _fenced(B * Nq, 768)
    fkv, dKV = _fenced(B * Nk, 512)
    fs = torch.full((hip.mha_bwd_keysplit_scratch_floats(B, Nq, Nk) + 64,), float("nan"), device=DEV)
    n_scr = fs.numel() - 64
    hip.mha_bwd_keysplit(q, k, v, do, dQKV[:, 256:512], dKV[:, :256], dKV[:, 256:], fs[:n_scr],
                         B, Nq, Nk, SCALE)
    torch.cuda.synchronize()
    refs = _mha_ref(q, k, v, do, B, Nq, Nk, SCALE, None)
    for nm, a, r in zip(("dq", "dk", "dv"), (dQKV[:, 256:512], dKV[:, :256], dKV[:, 256:]), refs):
        _within_rows("strided keysplit %s" % nm, a, r, C_MHA)
    bits = lambda t: t.contiguous().view(torch.int32)
    for name, t in (("dq's foreign columns", dQKV[:, :256]), ("dq's foreign columns", dQKV[:, 512:]),
                    ("dq fence", fq[-64:]), ("dk / dv fence", fkv[-64:]), ("scratch fence", fs[-64:])):
        assert bool((bits(t) == NAN_BITS).all()), "%s were written" % name


def test_refusals_one_by_one(hip):
    B, Nq, Nk = 1, 5, 40
    g = _gen(3)
    q, k, v, do = (_randn(g, B * n, 256) for n in (Nq, Nk, Nk, Nq))
    dq, dk, dv = (torch.full((B * n, 256), float("nan"), device=DEV) for n in (Nq, Nk, Nk))
    need = hip.mha_bwd_keysplit_scratch_floats(B, Nq, Nk)
    scr = torch.full((need,), float("nan"), device=DEV)
    fn = hip.lib().pn_mha_bwd_keysplit_f32
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = [t.data_ptr() for t in (q, k, v, do, dq, dk, dv)]

    def call(ptrs=ptrs, lds=(256,) * 7, scratch=scr.data_ptr(), floats=need, B=B, Nq=Nq, Nk=Nk):
        args = []
        for p, ld in zip(ptrs, lds):
            args += [p, ld]
        return fn(*args, scratch, floats, B, Nq, Nk, SCALE, stream)

    bad = []
    for j in range(7):
        bad.append(("null pointer %d" % j, dict(ptrs=ptrs[:j] + [None] + ptrs[j + 1:])))
        bad.append(("unaligned base %d" % j, dict(ptrs=ptrs[:j] + [ptrs[j] + 4] + ptrs[j + 1:])))
        for ld in (252, 258):
            bad.append(("stride %d of operand %d" % (ld, j),
                        dict(lds=(256,) * j + (ld,) + (256,) * (6 - j))))
    bad += [("null scratch", dict(scratch=None)), ("unaligned scratch", dict(scratch=scr.data_ptr() + 4)),
            ("scratch one float short", dict(floats=need - 1)), ("B = 0", dict(B=0)),
            ("B = 65536", dict(B=65536, floats=1 << 40)), ("Nq = 0", dict(Nq=0)),
            ("Nq < 0", dict(Nq=-1)), ("Nk = 0", dict(Nk=0))]
    for what, kw in bad:
        assert call(**kw) == -1, "%s was accepted" % what
    torch.cuda.synchronize()
    for t in (dq, dk, dv, scr):                      # nothing was launched
        assert bool((t.view(torch.int32) == NAN_BITS).all())
    with pytest.raises(RuntimeError):                # the binding passes the buffer's own size on
        hip.mha_bwd_keysplit(q, k, v, do, dq, dk, dv, scr[:need - 1], B, Nq, Nk, SCALE)
    assert call() == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (dq, dk, dv))
