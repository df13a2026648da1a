"""GPU: `pn_mha_bwd_keysplit_masked_f32` (csrc/attn_grad.hip), the key-split attention backward under
the forward's packed boolean mask, against float64 autograd (`test_grad_kernels_gpu._mha_ref` with
allowed = ~mask | mask.all(-1)) under that file's softmax-type row bound with the project's own
constant C_MHA = 115 (not retuned to this kernel).  The masks are packed by `hip.mask_pack`.  Every
case also runs `pn_mha_bwd_f32` under the same bits, prints both worst ratios and checks that the two
kernels differ by at most the sum of their two bounds; two launches of the new kernel agree bit for
bit; NaN-prefilled outputs are fully overwritten.  Shapes around the key chunk
c = hip.MHA_KEYSPLIT_CHUNK; the row patterns put whole chunks under the mask (the chunk maximum is
-inf there), and once the finest memory level of an 800 x 1333 image with 95 % of the keys masked."""
import pytest
import torch

from pairnet_amd.hip import MHA_KEYSPLIT_CHUNK as c
from test_grad_kernels_gpu import (C_MHA, DEV, FLT_MIN, U, _gen, _mha_ref, _randn, _within_rows,
                                   hip)  # noqa: F401  (`hip`: that module's fixture)

pytestmark = pytest.mark.gpu
SCALE = 32 ** -0.5
NAN_BITS = 0x7fc00000

# (B, Nq, Nk, share of masked keys in the random rows, with the row patterns below)
CASES = [(1, 1, 1, 0.5, False), (2, 9, 33, 0.5, False), (1, 100, c + 1, 0.5, True),
         (2, 37, 3 * c + 5, 0.5, True), (1, 130, 2 * c, 0.5, False), (1, 100, 16700, 0.95, False)]


def _ratio(got, ref):
    """Worst |got - ref| / (2^-24 max |ref row|) beyond FLT_MIN, without asserting."""
    ref = ref.to(DEV).double()
    err = (got.double() - ref).abs()
    mag = ref.abs().amax(-1, keepdim=True).expand_as(ref)
    r = torch.where(err <= FLT_MIN, torch.zeros_like(err), (err - FLT_MIN).clamp_min(0) / (U * mag))
    return float(torch.nan_to_num(r, nan=0.0).max())      # (0 / 0: a reference row of zeros)


def _logits(g, B, Nq, Nk, share, patterns):
    """Mask logits [B * Nq, Nk] (negative = masked, as pn_mask_pack reads them): random rows with
    `share` of the keys masked and, with `patterns`, in every image
      rows 0, 5, 10, ...  all masked (rowall = 1: the bits are ignored),
      row 1               only the last key attendable,
      row 2               only key 0 attendable,
      row 3               the attendable keys all lie in chunk 1 (keys c .. min(2c, Nk) - 1),
      rows 4, 6           (Nk = c + 1) the last chunk's single key masked: chunk 1 is all masked."""
    lg = torch.rand(B * Nq, Nk, generator=g, device=DEV) - share
    lg = torch.where(lg == 0, torch.ones_like(lg), lg)
    if patterns:
        v = lg.view(B, Nq, Nk)
        v[:, ::5] = -v[:, ::5].abs() - 0.5
        v[:, 1] = -1.0
        v[:, 1, -1] = 1.0
        v[:, 2] = -1.0
        v[:, 2, 0] = 1.0
        in1 = torch.zeros(Nk, dtype=torch.bool, device=DEV)
        in1[c:2 * c] = True
        in1 &= (torch.arange(Nk, device=DEV) - c) % 3 != 1      # (key c itself stays attendable)
        v[:, 3] = torch.where(in1, 1.0, -1.0)
        if Nk == c + 1:
            v[:, 4, -1] = -1.0
            v[:, 6, -1] = -1.0
            v[:, 4, 7] = 1.0
            v[:, 6, c - 1] = 1.0
    return lg


def _pack(hip, lg, B, Nq, Nk):
    bits = torch.empty(B * Nq, (Nk + 31) // 32, dtype=torch.int32, device=DEV)
    rowall = torch.empty(B * Nq, dtype=torch.int32, device=DEV)
    hip.mask_pack(lg, bits, rowall, B * Nq, Nk)
    m = lg < 0
    allowed = (~m | m.all(-1, keepdim=True)).view(B, Nq, Nk)
    return bits, rowall, m, allowed


def _masked(hip, q, k, v, do, B, Nq, Nk, bits, rowall):
    dq, dk, dv = (torch.full((B * n, 256), float("nan"), device=DEV) for n in (Nq, Nk, Nk))
    scr = torch.empty(hip.mha_bwd_keysplit_scratch_floats(B, Nq, Nk), device=DEV)
    hip.mha_bwd_keysplit(q, k, v, do, dq, dk, dv, scr, B, Nq, Nk, SCALE, bits=bits, rowall=rowall)
    return dq, dk, dv


def _parent(hip, q, k, v, do, B, Nq, Nk, bits, rowall):
    dq, dk, dv = (torch.full((B * n, 256), float("nan"), device=DEV) for n in (Nq, Nk, Nk))
    scr = torch.empty(hip.mha_bwd_scratch_floats(B, Nq, Nk), device=DEV)
    hip.mha_bwd(q, k, v, do, dq, dk, dv, scr, B, Nq, Nk, SCALE, bits=bits, rowall=rowall)
    return dq, dk, dv


def _check_case(hip, tag, q, k, v, do, B, Nq, Nk, bits, rowall, allowed, agree=("dq", "dk", "dv")):
    got = _masked(hip, q, k, v, do, B, Nq, Nk, bits, rowall)
    got2 = _masked(hip, q, k, v, do, B, Nq, Nk, bits, rowall)
    par = _parent(hip, q, k, v, do, B, Nq, Nk, bits, rowall) if agree else (None,) * 3
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in got), "%s: non-finite output" % tag
    assert all(torch.equal(a, b) for a, b in zip(got, got2)), "two launches differ"
    refs = _mha_ref(q, k, v, do, B, Nq, Nk, SCALE, allowed)
    for nm, a, p, r in zip(("dq", "dk", "dv"), got, par, refs):     # every figure before any assertion
        print("%s %s: masked keysplit worst ratio %.3f%s"
              % (tag, nm, _ratio(a, r),
                 ", pn_mha_bwd_f32 worst ratio %.3f" % _ratio(p, r) if p is not None else ""))
    for nm, a, p, r in zip(("dq", "dk", "dv"), got, par, refs):
        _within_rows("%s masked keysplit %s" % (tag, nm), a, r, C_MHA)
        if nm not in agree:
            continue
        r64 = r.to(DEV).double()
        bound = 2 * (C_MHA * U * r64.abs().amax(-1, keepdim=True) + FLT_MIN)
        assert bool(((a.double() - p.double()).abs() <= bound).all()), \
            "%s %s: kernels disagree" % (tag, nm)
    return got, refs


@pytest.mark.parametrize("B,Nq,Nk,share,patterns", CASES)
def test_masked_keysplit_against_float64_and_the_parent_kernel(hip, B, Nq, Nk, share, patterns):
    g = _gen(B * 100000 + Nq * 1000 + Nk + 7)
    q, k, v = _randn(g, B * Nq, 256), _randn(g, B * Nk, 256), _randn(g, B * Nk, 256)
    do = _randn(g, B * Nq, 256)
    lg = _logits(g, B, Nq, Nk, share, patterns)
    bits, rowall, m, allowed = _pack(hip, lg, B, Nq, Nk)
    if patterns:
        assert int(rowall.sum()) == B * ((Nq + 4) // 5)
        mv = m.view(B, Nq, Nk)
        assert bool((~mv[:, 1]).sum(-1).eq(1).all()) and bool((~mv[:, 1, -1]).all())
        assert bool((~mv[:, 2]).sum(-1).eq(1).all()) and bool((~mv[:, 2, 0]).all())
        assert bool(mv[:, 3, :c].all()) and bool(mv[:, 3, 2 * c:].all()) and \
            bool((~mv[:, 3, c:2 * c]).any())
        if Nk == c + 1:
            assert bool(mv[:, 4, c:].all()) and bool(mv[:, 6, c:].all())
            assert bool((~mv[:, 4, :c]).any()) and bool((~mv[:, 6, :c]).any())
    if Nk == 16700:
        print("masked share %.4f" % float(m.float().mean()))
        assert 0.94 < float(m.float().mean()) < 0.96
    _check_case(hip, "B%d Nq%d Nk%d" % (B, Nq, Nk), q, k, v, do, B, Nq, Nk, bits, rowall, allowed)


def test_columns_masked_in_every_row_get_zero_bits(hip):
    """Keys masked in EVERY row (a whole chunk among them, and no rowall row): their dk / dv rows are
    written, and are exactly zero bits."""
    B, Nq, Nk = 2, 37, 3 * c + 5
    g = _gen(4242)
    q, k, v = _randn(g, B * Nq, 256), _randn(g, B * Nk, 256), _randn(g, B * Nk, 256)
    do = _randn(g, B * Nq, 256)
    lg = _logits(g, B, Nq, Nk, 0.5, False)
    dead = torch.zeros(Nk, dtype=torch.bool, device=DEV)
    dead[c:2 * c] = True                       # chunk 1 entirely
    dead[[0, 31, 32, c - 1, 2 * c, Nk - 1]] = True
    dead[2 * c + 40:2 * c + 90:3] = True
    lg[:, dead] = -1.0
    lg[:, 5] = 1.0                             # (every row keeps an attendable key)
    bits, rowall, m, allowed = _pack(hip, lg, B, Nq, Nk)
    assert int(rowall.sum()) == 0
    got, _ = _check_case(hip, "dead columns", q, k, v, do, B, Nq, Nk, bits, rowall, allowed)
    for nm, t in (("dk", got[1]), ("dv", got[2])):
        rows = t.view(B, Nk, 256)[:, dead]
        assert bool((rows.contiguous().view(torch.int32) == 0).all()), "%s rows of dead keys" % nm
        live = t.view(B, Nk, 256)[:, ~dead]
        assert bool((live.abs().amax(-1) > 0).all())


def test_no_mask_through_the_new_entry_is_the_old_entry_bit_for_bit(hip):
    B, Nq, Nk = 2, 37, 3 * c + 5
    g = _gen(99)
    q, k, v, do = (_randn(g, B * n, 256) for n in (Nq, Nk, Nk, Nq))
    need = hip.mha_bwd_keysplit_scratch_floats(B, Nq, Nk)
    old = [torch.full((B * n, 256), float("nan"), device=DEV) for n in (Nq, Nk, Nk)]
    new = [torch.full((B * n, 256), float("nan"), device=DEV) for n in (Nq, Nk, Nk)]
    scr = torch.empty(need, device=DEV)
    hip.mha_bwd_keysplit(q, k, v, do, *old, scr, B, Nq, Nk, SCALE)
    fn = hip.lib().pn_mha_bwd_keysplit_masked_f32
    args = []
    for t in (q, k, v, do, *new):
        args += [t.data_ptr(), 256]
    assert fn(*args, scr.data_ptr(), need, B, Nq, Nk, SCALE, None, None,
              torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for a, b in zip(old, new):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_masked_peaked_softmax(hip):
    """q scaled by 8 under a mask (as `test_attn_grad_kernels_gpu.test_peaked_softmax`): against
    float64 only -- pn_mha_bwd_f32 is outside its own bound on such an input (labnotes R23.2)."""
    B, Nq, Nk = 2, 37, 3 * c + 5
    g = _gen(88)
    q, k, v = _randn(g, B * Nq, 256, scale=8.0), _randn(g, B * Nk, 256), _randn(g, B * Nk, 256)
    do = _randn(g, B * Nq, 256)
    lg = _logits(g, B, Nq, Nk, 0.5, True)
    bits, rowall, m, allowed = _pack(hip, lg, B, Nq, Nk)
    _check_case(hip, "masked peaked", q, k, v, do, B, Nq, Nk, bits, rowall, allowed, agree=())


def _fenced(rows, ld, fence=64):
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
    lg = _logits(g, B, Nq, Nk, 0.5, True)
    bits, rowall, m, allowed = _pack(hip, lg, B, Nq, Nk)
    fq, dQKV = _fenced(B * Nq, 768)
    fkv, dKV = _fenced(B * Nk, 512)
    fs = torch.full((hip.mha_bwd_keysplit_scratch_floats(B, Nq, Nk) + 64,), float("nan"), device=DEV)
    n_scr = fs.numel() - 64
    hip.mha_bwd_keysplit(q, k, v, do, dQKV[:, 256:512], dKV[:, :256], dKV[:, 256:], fs[:n_scr],
                         B, Nq, Nk, SCALE, bits=bits, rowall=rowall)
    torch.cuda.synchronize()
    refs = _mha_ref(q, k, v, do, B, Nq, Nk, SCALE, allowed)
    for nm, a, r in zip(("dq", "dk", "dv"), (dQKV[:, 256:512], dKV[:, :256], dKV[:, 256:]), refs):
        _within_rows("strided masked keysplit %s" % nm, a, r, C_MHA)
    ib = lambda t: t.contiguous().view(torch.int32)
    for name, t in (("dq's foreign columns", dQKV[:, :256]), ("dq's foreign columns", dQKV[:, 512:]),
                    ("dq fence", fq[-64:]), ("dk / dv fence", fkv[-64:]), ("scratch fence", fs[-64:])):
        assert bool((ib(t) == NAN_BITS).all()), "%s were written" % name


def test_one_mask_operand_without_the_other_is_refused(hip):
    B, Nq, Nk = 1, 5, 40
    g = _gen(3)
    q, k, v, do = (_randn(g, B * n, 256) for n in (Nq, Nk, Nk, Nq))
    dq, dk, dv = (torch.full((B * n, 256), float("nan"), device=DEV) for n in (Nq, Nk, Nk))
    need = hip.mha_bwd_keysplit_scratch_floats(B, Nq, Nk)
    scr = torch.full((need,), float("nan"), device=DEV)
    bits, rowall, _, _ = _pack(hip, _logits(g, B, Nq, Nk, 0.5, False), B, Nq, Nk)
    fn = hip.lib().pn_mha_bwd_keysplit_masked_f32
    stream = torch.cuda.current_stream().cuda_stream
    args = []
    for t in (q, k, v, do, dq, dk, dv):
        args += [t.data_ptr(), 256]
    tail = lambda b, r: (scr.data_ptr(), need, B, Nq, Nk, SCALE, b, r, stream)
    assert fn(*args, *tail(bits.data_ptr(), None)) == -1
    assert fn(*args, *tail(None, rowall.data_ptr())) == -1
    torch.cuda.synchronize()
    for t in (dq, dk, dv, scr):                      # nothing was launched
        assert bool((t.view(torch.int32) == NAN_BITS).all())
    for kw in (dict(bits=bits), dict(rowall=rowall)):
        with pytest.raises(RuntimeError):
            hip.mha_bwd_keysplit(q, k, v, do, dq, dk, dv, scr, B, Nq, Nk, SCALE, **kw)
    assert fn(*args, *tail(bits.data_ptr(), rowall.data_ptr())) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (dq, dk, dv))
