"""GPU: the deterministic deformable-attention backward (`pn_msda_bwd_det_f32`,
csrc/msda_grad.hip) -- accuracy against float64 autograd, the summation ORDER of its definition
(bit for bit against tests/msda_det_ref.py), reproducibility with a reused dirty scratch,
accumulation into the caller's buffer, and the mmcv-shaped surface.  Every call runs with 256 guard
bytes in front of and behind each output and the scratch."""
import functools

import pytest
import torch

import fwd_cases
import msda_det_ref as R
from oracle import layers as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
PATTERN = 0xA5

# the four small pyramids of tests/test_kernels_gpu.py::test_mmcv_shaped_msda_backward
CASES = [([(3, 4), (6, 8), (12, 16)], 2, 252),
         ([(5, 7)], 1, 1),
         ([(2, 3), (4, 5), (7, 9), (13, 17)], 2, 301),
         ([(9, 1), (17, 3)], 3, 100)]


@pytest.fixture(scope="module")
def hip(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip as h
    h.lib()
    return h


class Guarded:
    """A device buffer of `nbytes` with GUARD pattern bytes on either side."""

    def __init__(self, nbytes, fill=0):
        self.raw = torch.full((nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.body = self.raw[GUARD:GUARD + nbytes]
        self.body.fill_(fill)

    def f32(self, *shape):
        return self.body.view(torch.float32).view(*shape)

    def intact(self):
        return bool((self.raw[:GUARD] == PATTERN).all()) and bool((self.raw[-GUARD:] == PATTERN).all())


def _levels(shapes):
    ss = torch.tensor(shapes, dtype=torch.int64)
    return ss, torch.cat([ss.new_zeros(1), (ss[:, 0] * ss[:, 1]).cumsum(0)[:-1]])


def run_det(hip, inp, scratch=None, into=None, prefill=None):
    """One guarded pn_msda_bwd_det_f32 call on the inputs `inp` (device tensors) -> (grad_value,
    grad_loc, grad_aw) as fresh tensors.  `into`: a Guarded grad_value to accumulate into."""
    value, ss, starts, loc, aw, gout = (inp[k] for k in ("value", "ss", "starts", "loc", "aw", "gout"))
    B, N = value.shape[:2]
    Nq, Lv = loc.shape[1], loc.shape[3]
    gv = into if into is not None else Guarded(value.numel() * 4)
    if prefill is not None:
        gv.f32(*value.shape).fill_(prefill)
    gl, ga = Guarded(loc.numel() * 4, 0x7F), Guarded(aw.numel() * 4, 0x7F)    # (overwritten)
    if scratch is None:
        scratch = Guarded(hip.msda_bwd_det_scratch_bytes(B, N, Nq, Lv), 0xC3)  # (arrives dirty)
    hip.msda_bwd_det(value, 256, ss, starts, loc, aw, gout, gv.f32(*value.shape), gl.f32(*loc.shape),
                     ga.f32(*aw.shape), B, N, Nq, Lv, scratch=scratch.body)
    torch.cuda.synchronize()
    for name, g in (("grad_value", gv), ("grad_sampling_loc", gl), ("grad_attn_weight", ga),
                    ("scratch", scratch)):
        assert g.intact(), "guard bytes around %s were written" % name
    return gv.f32(*value.shape).clone(), gl.f32(*loc.shape).clone(), ga.f32(*aw.shape).clone()


@functools.lru_cache(maxsize=None)
def case(idx):
    """Inputs of CASES[idx] (planted pixels on heads 0-3 of every query: long lists), the float64
    autograd reference of grad_value, and the atomic entry's other two outputs.  Computed once."""
    from pairnet_amd import hip
    shapes, B, Nq = CASES[idx]
    value = fwd_cases.msda_value(B, shapes, 60 + idx)
    loc, aw = fwd_cases.msda_locations(B, shapes, Nq, 70 + idx)
    gout = torch.randn(B, Nq, 256, generator=torch.Generator().manual_seed(80 + idx))
    v, l, a = (t.double().clone().requires_grad_(True) for t in (value, loc, aw))
    L.msda_core(v, shapes, l, a).backward(gout.double())
    ss, starts = _levels(shapes)
    inp = {k: t.to(DEV).contiguous() for k, t in dict(value=value, ss=ss, starts=starts, loc=loc,
                                                       aw=aw, gout=gout).items()}
    N = value.shape[1]
    gv, gl, ga = torch.zeros_like(inp["value"]), torch.empty_like(inp["loc"]), torch.empty_like(inp["aw"])
    hip.msda_bwd(inp["value"], 256, inp["ss"], inp["starts"], inp["loc"], inp["aw"], inp["gout"], gv,
                 gl, ga, B, N, Nq, len(shapes))
    torch.cuda.synchronize()
    return dict(inp=inp, ref_gv=v.grad.float(), atomic=(gv, gl, ga), shapes=shapes, B=B, N=N, Nq=Nq)


@functools.lru_cache(maxsize=None)
def det_result(idx):
    from pairnet_amd import hip
    return run_det(hip, case(idx)["inp"])


def _rel_err(got, want):
    return float((got.cpu().double() - want.double()).abs().max()) / max(float(want.abs().max()), 1e-30)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_accuracy_and_the_other_two_outputs(hip, idx):
    """grad_value within 1e-4 of the largest float64 reference entry (the bound the atomic kernel is
    held to); grad_sampling_loc / grad_attn_weight bit for bit the atomic entry's."""
    c = case(idx)
    gv, gl, ga = det_result(idx)
    err = _rel_err(gv, c["ref_gv"])
    print("case %d: grad_value max err / max |ref| = %.3e (atomic entry: %.3e)"
          % (idx, err, _rel_err(c["atomic"][0], c["ref_gv"])))
    assert err < 1e-4
    assert torch.equal(gl, c["atomic"][1])
    assert torch.equal(ga, c["atomic"][2])


@pytest.mark.parametrize("kw", [dict(seed=0), dict(seed=1),
                                dict(seed=3, nq=300, xs=(2.5, 3.0), ys=(1.0,))],
                         ids=["short-lists", "short-lists-2", "lists-of-1200"])
def test_summation_order_is_the_definitions(hip, kw):
    """Every product is exact on these inputs, so only the ORDER of the additions decides the fp32
    sums: ascending id, as tests/msda_det_ref.py adds them on the host.  The third input piles
    1 200 records on single destinations: the path for lists past the LDS capacity."""
    oc = R.order_case(**kw)
    inp = {k: oc[k].to(DEV) for k in ("value", "ss", "starts", "loc", "aw", "gout")}
    gv, _, _ = run_det(hip, inp)
    bad = (gv.cpu() != oc["expected"]).flatten(2).any(-1).nonzero().tolist()
    assert not bad, "destinations (b, token, head) off the ascending-id sum: %s" % bad[:8]
    assert torch.equal(gv.cpu(), oc["expected"])


@pytest.mark.parametrize("idx", [0, 2])
def test_reproducible_with_a_reused_dirty_scratch(hip, idx):
    c = case(idx)
    scratch = Guarded(hip.msda_bwd_det_scratch_bytes(c["B"], c["N"], c["Nq"], len(c["shapes"])), 0x00)
    first = run_det(hip, c["inp"], scratch=scratch)
    scratch.body.fill_(0xFF)
    second = run_det(hip, c["inp"], scratch=scratch)
    third = run_det(hip, c["inp"], scratch=scratch)
    for a, b_, c_ in zip(first, second, third):
        assert torch.equal(a, b_) and torch.equal(a, c_)
    assert torch.equal(first[0], det_result(idx)[0])          # (and with a scratch of its own)


def test_accumulates_into_the_callers_buffer(hip):
    c = case(0)
    first = det_result(0)[0]
    acc = Guarded(first.numel() * 4)
    run_det(hip, c["inp"], into=acc)
    twice, _, _ = run_det(hip, c["inp"], into=acc)
    assert torch.equal(twice, 2 * first)


def test_untouched_destinations_are_not_written(hip):
    """Locations inside one corner of level 1 (pixels x <= 2, y <= 2 of the 6 x 8 map), every other
    level's far outside: all other tokens keep their pre-filled 7.0 bit for bit, the touched ones
    hold 7.0 + the sum (one rounding)."""
    shapes, B, Nq = CASES[0]
    c = case(0)
    g = torch.Generator().manual_seed(5)
    loc = torch.full((B, Nq, 8, 3, 4, 2), -5.0)
    loc[:, :, :, 1] = torch.rand(B, Nq, 8, 4, 2, generator=g) * 0.25 + 0.05
    inp = dict(c["inp"], loc=loc.to(DEV))
    zero_based, _, _ = run_det(hip, inp)
    got, _, _ = run_det(hip, inp, prefill=7.0)
    touched = torch.zeros(c["N"], dtype=torch.bool)
    for y in range(3):
        touched[12 + y * 8:12 + y * 8 + 3] = True
    assert bool((zero_based.cpu()[:, ~touched] == 0).all())
    assert bool((zero_based.cpu()[:, touched] != 0).any())
    assert bool((got.cpu()[:, ~touched] == 7.0).all())
    assert torch.equal(got, zero_based + 7.0)


def test_mmcv_surface(hip):
    from pairnet_amd.mmcv_ops import MultiScaleDeformableAttnFunction, ms_deform_attn_backward
    c = case(0)
    i = c["inp"]
    gv, gl, ga = (torch.zeros_like(i[k]) for k in ("value", "loc", "aw"))
    ms_deform_attn_backward(i["value"], i["ss"], i["starts"], i["loc"], i["aw"], i["gout"], gv, gl, ga,
                            64, deterministic=True)
    want = det_result(0)
    assert torch.equal(gv, want[0]) and torch.equal(gl, want[1]) and torch.equal(ga, want[2])
    # deterministic=False decides too, whatever torch's switch says: the atomic entry's other outputs
    ms_deform_attn_backward(i["value"], i["ss"], i["starts"], i["loc"], i["aw"], i["gout"],
                            torch.zeros_like(gv), gl, ga, 64, deterministic=False)
    assert torch.equal(gl, c["atomic"][1])
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        grads = []
        for _ in range(2):
            v = i["value"].clone().requires_grad_(True)
            out = MultiScaleDeformableAttnFunction.apply(v, i["ss"], i["starts"], i["loc"], i["aw"], 64)
            out.backward(i["gout"])
            grads.append(v.grad)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert torch.equal(grads[0], grads[1])
    assert torch.equal(grads[0], want[0])
