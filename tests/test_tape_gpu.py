"""GPU: `Tape._lin_bwd` (pair-net_amd/tape.py) at an output width that is no multiple of 4 -- the
class heads' 134 logits, 57 or 50 relations.  Four tapes used to pad such a layer by hand around
the multiple-of-4 `_lin_bwd`; that composition is restated here (`_old_composition`) and the
method must give the same bits, whether it is handed dy N-wide or already padded, at a row offset
inside the parameter, with and without a bias.  The values are also held against a float64
statement, at the project's gradient criterion: 1e-5 of the statement's largest entry."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, K = 33, 8           # M: no multiple of the dW GEMM's 32-deep k-chunks


@pytest.fixture(scope="module")
def tape(built_lib):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from pairnet_amd import hip
    from pairnet_amd.tape import Tape
    hip.lib()

    class BareTape(Tape):
        """The shared steps alone: no module, no layout."""

        def __init__(self):
            self.dev = torch.device(DEV)

    return BareTape()


def _old_composition(tape, dy, x, W, grads, wname, bname, row0):
    """What `_cls_backward`, `BBoxTailGrad._lin_bwd`, `SegmenterHeadGrad.backward` and
    `BaselineHeadGrad._lin_bwd_pad4` did: zero-pad dy and W to the next multiple of 4, take the
    gradients at that width into zeroed buffers, add their first N rows on."""
    from pairnet_amd import hip
    N = W.shape[0]
    Np = (N + 3) // 4 * 4
    zeros = lambda *s: torch.zeros(*s, device=DEV, dtype=torch.float32)
    dyp, Wp = zeros(M, Np), zeros(Np, K)
    dyp[:, :N].copy_(dy)
    Wp[:N].copy_(W)
    gp = {"W": zeros(Np, K), "b": zeros(Np)}
    dx = tape._lin_bwd(dyp, x, Wp, gp, "W", None if bname is None else "b")    # Np % 4 == 0
    gw = grads[wname][row0:row0 + N]
    hip.add_periodic(gw, gp["W"][:N], gw)
    if bname is not None:
        gb = grads[bname][row0:row0 + N]
        hip.add_periodic(gb, gp["b"][:N], gb)
    return dx


@pytest.mark.parametrize("padded_dy", [False, True])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("row0", [0, 4])
@pytest.mark.parametrize("N", [1, 3, 5, 50, 4])          # 4: the unpadded control
def test_lin_bwd_ragged(tape, N, row0, bias, padded_dy):
    g = torch.Generator(device=DEV).manual_seed(1000 * N + 10 * row0 + 2 * bias + padded_dy)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    dy, x, W = r(M, N), r(M, K), r(N, K)
    rows = row0 + N + 3                                  # the parameter has rows on both sides
    prev = {"w": r(rows, K), "b": r(rows)}
    bname = "b" if bias else None
    given = dy
    if padded_dy:
        given = torch.zeros(M, (N + 3) // 4 * 4, device=DEV)
        given[:, :N].copy_(dy)
    new, old = ({k: v.clone() for k, v in prev.items()} for _ in range(2))
    dx_new = tape._lin_bwd(given, x, W, new, "w", bname, row0=row0)
    dx_old = _old_composition(tape, dy, x, W, old, "w", bname, row0)
    torch.cuda.synchronize()
    for name, a, b in (("dW", new["w"], old["w"]), ("db", new["b"], old["b"]), ("dx", dx_new, dx_old)):
        assert torch.equal(a, b), "%s differs from the old composition by up to %.3e" % (
            name, float((a - b).abs().max()))
    # float64: the N rows at row0 get dy^T x / the column sums added, every other row is untouched
    d64, x64, W64 = dy.double(), x.double(), W.double()
    want_w, want_b = prev["w"].double(), prev["b"].double()
    want_w[row0:row0 + N] += d64.T @ x64
    if bias:
        want_b[row0:row0 + N] += d64.sum(0)
    for name, got, want in (("dW", new["w"], want_w), ("db", new["b"], want_b),
                            ("dx", dx_new, d64 @ W64)):
        err, top = float((got.double() - want).abs().max()), float(want.abs().max())
        print("N=%d row0=%d bias=%d padded=%d %s: max |err| %.3e, largest entry %.3e"
              % (N, row0, bias, padded_dy, name, err, top))
        assert tuple(got.shape) == tuple(want.shape) and err <= 1e-5 * top, (name, err, top)
    outside = torch.ones(rows, dtype=torch.bool, device=DEV)
    outside[row0:row0 + N] = False
    assert torch.equal(new["w"][outside], prev["w"][outside])
    assert torch.equal(new["b"][outside], prev["b"][outside])
    if not bias:
        assert torch.equal(new["b"], prev["b"])
