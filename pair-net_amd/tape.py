"""What every backward tape shares (grad.py, pixel_grad.py, backbone_grad.py, seg_grad.py): the
taped module on its device, the flat gradient buffer with its layout, and the three backward steps
all of them are composed of -- a linear layer's (`_lin_bwd`), LayerNorm(256)'s (`_ln_bwd`) and the
in-place sum (`_acc`).  A tape class says which parameters it differentiates, in the order its
`backward` completes them (`param_groups`), and walks its own part of the network."""
from collections import OrderedDict

import torch

from . import hip

__all__ = ["Tape"]


class Tape:
    """tape = SomeGrad(module, flat=None, base=0): `module` is a head or a backbone on an MI355X
    (`self.module`; the head tapes also name it `self.head`, the backbone tapes `self.backbone`).
    `self.t` is the tape of the last forward (None before it)."""

    # `_zero_grads` clears the flat buffer unless this is set: a tape whose backward() runs its
    # parent's walk inside its own sets it around that call, so that the buffer is zeroed once
    _zeroed = False

    def __init__(self, module, flat=None, base=0):
        """`flat`, `base`: keep the gradients in flat[base : base + flat_numel] of a caller-owned
        buffer (several tapes sharing one buffer: one optimizer launch, one reducer)."""
        if module.device is None or module.device.type != "cuda":
            raise RuntimeError("%s needs its module on an MI355X (.to('cuda:N')); there is no CPU "
                               "path" % type(self).__name__)
        if module.w is None:
            module._pack()
        self.module, self.dev = module, module.device
        self.t = None
        self._build_layout(module, flat, base)

    def _build_layout(self, head, flat, base):
        """Every gradient is a view of ONE flat buffer, parameters in the order their gradients are
        COMPLETED by backward() (rel_cls_embed, relation layers last to first, the relation
        embeddings, the Matrix Learner, the two PPN MLPs, then the optional class path): the
        optimizer runs over it in one launch and a data-parallel reducer can all-reduce a
        finished prefix while the rest of the backward pass is still running (train.py, dist.py)."""
        self.layout, off = OrderedDict(), 0
        self.group_end = OrderedDict()           # group name -> end offset of its last segment
        for group, names in self.param_groups(head):
            for n in names:
                shape = tuple(head._params[n].shape)
                numel = int(torch.Size(shape).numel())
                self.layout[n] = (off, shape, numel)
                off += (numel + 63) // 64 * 64
            self.group_end[group] = off
        self.flat_numel = off
        if flat is None:
            self.flat_grad = torch.zeros(off, device=self.dev, dtype=torch.float32)
        else:
            self.flat_grad = flat[base:base + off]
            assert self.flat_grad.numel() == off and base % 64 == 0
        self.grads = {n: self.flat_grad[o:o + k].view(shape)
                      for n, (o, shape, k) in self.layout.items()}

    @classmethod
    def size_of(cls, head):
        """Floats of the flat gradient buffer of this tape for `head` (segments padded to 64)."""
        return sum((int(torch.Size(tuple(head._params[n].shape)).numel()) + 63) // 64 * 64
                   for _, names in cls.param_groups(head) for n in names)

    @staticmethod
    def param_groups(module):
        """[(group, [reference parameter names])] in the order backward() completes them."""
        raise NotImplementedError

    # ------------------------------------------------------------------ small helpers
    def _E(self, *shape):
        return torch.empty(*shape, device=self.dev, dtype=torch.float32)

    def _zeros(self, *shape):
        return torch.zeros(*shape, device=self.dev, dtype=torch.float32)

    def _acc(self, a, b):
        hip.add_periodic(a, b, a)

    def _zero_grads(self):
        if not self._zeroed:
            self.flat_grad.zero_()
        return self.grads

    def _lin_bwd(self, dy, x, W, grads, wname, bname, row0=0, need_dx=True):
        """y = x W^T + b.  dy [M, N] (row stride free), x [M, K] contiguous, W [N, K] rows of a
        reference parameter (`row0`: their offset inside it).  Accumulates d W / d b into
        grads[wname][row0:row0+N] / grads[bname][row0:row0+N]; returns d x [M, K] or None.

        The GEMMs contract over multiples of 4.  An output width N that is none (the class heads:
        134 logits, 57 or 50 relations) is padded with zero columns of dy and zero rows of W to
        the next one, Np, the gradients are taken at that width into zeroed buffers and their
        first N rows added on; a `dy` that is already [M, Np] with zero columns behind the N-th
        (a caller that scatters into it) is taken as it is."""
        M, K = x.shape
        N = W.shape[0]
        Np = (N + 3) // 4 * 4
        if Np != N:
            dyp = dy
            if dy.shape[1] != Np:
                dyp = self._zeros(M, Np)
                dyp[:, :N].copy_(dy)
            Wp = self._zeros(Np, K)
            Wp[:N].copy_(W)
            gp = {"W": self._zeros(Np, K)}
            if bname is not None:
                gp["b"] = self._zeros(Np)
            dx = self._lin_bwd(dyp, x, Wp, gp, "W", bname and "b", 0, need_dx)
            self._acc(grads[wname][row0:row0 + N], gp["W"][:N])
            if bname is not None:
                self._acc(grads[bname][row0:row0 + N], gp["b"][:N])
            return dx
        assert K % 4 == 0, (M, N, K)
        # the dW contraction runs over M: padded with zero rows to whole 32-deep k-chunks of the
        # GEMM kernels (no ragged-tail slow path; M % 4 == 0 is required anyway)
        Mp = (M + 31) // 32 * 32
        dyw = dy
        if Mp != M:
            dyw = torch.zeros(Mp, N, device=self.dev, dtype=torch.float32)
            dyw[:M].copy_(dy)
        xt = self._E(K, Mp)
        hip.transpose(x, xt)                   # (columns M .. Mp-1 zero-filled)
        gw = grads[wname][row0:row0 + N]
        tmp = self._E(N, K)
        # dW[n][k] = sum_m dy[m][n] x[m][k]: A = dy read column-major, "W" operand = x^T;
        # a long contraction over few output tiles is split (deterministic split-K + reduce)
        # (few output tiles, tens of thousands of rows to contract: 16 K-slices on the 64x64 tile
        # kernel instead of the 32x32 skinny kernel's 64 workgroups -- 134 -> ~30 us at 21 950 rows)
        kw = dict(scratch=self._E(16 * N * K), force="tile64", ksplit=16) if Mp >= 2048 else {}
        hip.gemm(dyw, xt, tmp, M=N, N=K, K=Mp, lda=dyw.stride(0), ldw=Mp, ldc=K, colmajor=True, **kw)
        hip.add_periodic(gw, tmp, gw)
        if bname is not None:
            hip.colsum(dy, grads[bname][row0:row0 + N], accumulate=True)
        if not need_dx:
            return None
        Wt = self._E(K, N)
        hip.transpose(W, Wt)
        dx = self._E(M, K)
        hip.gemm(dy, Wt, dx, M=M, N=K, K=N, lda=dy.stride(0), ldw=N, ldc=K)
        return dx

    def _ln_bwd(self, dy, x, prefix, grads):
        """LayerNorm(256) backward from its saved input; accumulates d weight / d bias."""
        w = self.module.w
        dx, gx = self._E(*x.shape), self._E(*x.shape)
        hip.layernorm256_bwd(dy, x, w[prefix + "weight"], dx, gx)
        hip.colsum(gx, grads[prefix + "weight"], accumulate=True)
        hip.colsum(dy, grads[prefix + "bias"], accumulate=True)
        return dx
