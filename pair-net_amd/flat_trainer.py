"""What the three training steps share (`TailTrainer` train.py, `BaselineTrainer`
baseline_train.py, `BBoxTrainer` bbox_train.py): `FlatTrainer` owns ONE flat gradient buffer that
every tape writes into, the flat parameter / moment buffers of the same layout that the head's
device weights alias, the per-segment multipliers, the clip + (guarded) AdamW launch, the
learning-rate schedule and `write_back()`; the `refresh_*` functions below rewrite, in place, the
weight packs the INFERENCE kernels read that are functions of trained parameters (captured
hipGraphs keep their pointers).  A subclass says which tapes, which names are frozen / repacked /
aliased and which multiplier rule, writes its own `step()`, and lists the `refresh_*` calls its
head needs in `_refresh_derived()`."""
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import hip

__all__ = ["FlatTrainer", "step_lr"]


def step_lr(base_lr, epoch, steps=(5, 10), gamma=0.5):
    """mmcv's StepLrUpdaterHook by epoch (`lr_config = dict(policy="step", gamma=0.5, step=[5, 10])`,
    configs/mask2former/pairnet.py:370): the learning rate of 0-based `epoch`."""
    return base_lr * gamma ** sum(1 for s in steps if epoch >= s)


class FlatTrainer:
    LR_STEPS, LR_GAMMA = (5, 10), 0.5      # `set_epoch`'s defaults
    reducer = None                         # a `dist.GradReducer` over `flat_grad`, where there is one

    def __init__(self, head, segments, multipliers, backbone=None, lr=1e-4, weight_decay=1e-4,
                 betas=(0.9, 0.999), eps=1e-8, max_norm=0.1, frozen=(), repacked=(), aliases=None):
        """`segments`: [(attribute, name prefix, tape class, the module it tapes)] in buffer order;
        each tape becomes `self.<attribute>` (`tape`, `pd_tape`, `bb_tape`; None where absent) and
        its names enter the layout behind the prefix ("" for the head, "backbone.").
        `multipliers(names, frozen)` -> (lr multipliers, decay multipliers), one per layout name.
        `frozen`: names that stay in the layout with multipliers 0 -- value copied into `flat_p`,
        not in `params`, not aliased.  `repacked`: names whose `head.w[...]` holds another layout
        (refreshed, not aliased).  `aliases`: {further key of `head.w`: name}."""
        from .plans import PlanCache
        self.head, self.backbone = head, backbone
        self.lr, self.wd, self.betas, self.eps, self.max_norm = lr, weight_decay, betas, eps, max_norm
        if head.w is None:
            head._pack()
        dev = self.dev = self.device = head.device
        if backbone is not None:
            if backbone.device is None:
                backbone.to(dev)
            if backbone.w is None:
                backbone._pack()
        # plans captured so far bake the addresses of the weight tensors that are re-homed below
        # into their hipGraphs: start from fresh plans (the arenas, shape-dependent only, stay)
        head._plans = PlanCache(head._plans.max_plans)
        # ---- ONE flat gradient buffer for every tape, segment after segment ----
        sizes = [cls.size_of(module) for _, _, cls, module in segments]
        self._seg_span = [(sum(sizes[:i]), n) for i, n in enumerate(sizes)]
        self.n = sum(sizes)
        self.flat_grad = torch.zeros(self.n, device=dev, dtype=torch.float32)
        self.tape = self.pd_tape = self.bb_tape = None
        self.layout = OrderedDict()        # name -> (offset in the shared buffer, shape, numel)
        src = {}                           # where a parameter's value lives
        for (attr, prefix, cls, module), (base, _) in zip(segments, self._seg_span):
            tape = cls(module, flat=self.flat_grad, base=base)
            setattr(self, attr, tape)
            for n, (o, shape, k) in tape.layout.items():
                self.layout[prefix + n] = (o + base, shape, k)
                src[prefix + n] = module._params[n]
        frozen = set(frozen)
        self.names = [n for n in self.layout if n not in frozen]
        # ---- flat parameters; the head's device weights become views of them ----
        self.flat_p = torch.zeros(self.n, device=dev, dtype=torch.float32)
        self.flat_m = torch.zeros_like(self.flat_p)
        self.flat_v = torch.zeros_like(self.flat_p)
        w = head.w
        self.params = OrderedDict()
        self._repacked = set(repacked)
        for n, (o, shape, k) in self.layout.items():
            view = self.flat_p[o:o + k].view(shape)
            view.copy_(src[n].to(dev))
            if n in frozen:
                continue
            self.params[n] = view
            if n.startswith("backbone."):
                continue          # the backbone's packed weights are all derived (BatchNorm folded)
            if n not in self._repacked:
                # same bytes as the reference layout (ConvTiny's first layer: [64,1,7,7] == [64,49],
                # the 1x1 convolutions: [256,C,1,1] == [256,C])
                w[n] = view.view(w[n].shape)
        for alias, n in (aliases or {}).items():
            w[alias] = w[n]
        # ---- per-segment multipliers (mmcv paramwise_cfg) ----
        lrs, wds = multipliers(self.layout, frozen)
        offs = [o for o, _, _ in self.layout.values()] + [self.n]
        self.seg_off = torch.tensor(offs, dtype=torch.int64, device=dev)
        self.seg_lr = torch.tensor(lrs, dtype=torch.float32, device=dev)
        self.seg_wd = torch.tensor(wds, dtype=torch.float32, device=dev)
        self.clip = torch.zeros(2, device=dev, dtype=torch.float32)     # [grad norm, coefficient]
        self._scratch = torch.zeros(256, device=dev, dtype=torch.float64)
        self.steps = 0
        self._w_dicts = (head.w, backbone.w if backbone is not None else None)
        self._refresh_derived()

    def _refresh_derived(self):
        raise NotImplementedError

    def _check_not_repacked(self):
        """load_state_dict / an in-place parameter update made a module re-pack its device weights:
        the flat buffers of this trainer no longer back them."""
        if self.head.w is not self._w_dicts[0] or (self.backbone is not None
                                                   and self.backbone.w is not self._w_dicts[1]):
            raise RuntimeError("the head (or backbone) re-packed its weights since this %s was built "
                               "(load_state_dict, parameter update, .to()): build a new one"
                               % type(self).__name__)

    def _ready(self, i):
        """The `on_ready` hook of segment i's tape: its ends, as ends in the whole buffer."""
        base, n = self._seg_span[i]
        return lambda end: self._gradients_ready(base + min(end, n))

    def _gradients_ready(self, end):
        self.reducer.ready(end)

    def set_epoch(self, epoch, steps=None, gamma=None):
        """The config's learning-rate schedule (step policy by 0-based epoch; the class's
        `LR_STEPS` / `LR_GAMMA` unless given): sets `self.lr`."""
        if not hasattr(self, "base_lr"):
            self.base_lr = self.lr
        self.lr = step_lr(self.base_lr, epoch, self.LR_STEPS if steps is None else steps,
                          self.LR_GAMMA if gamma is None else gamma)
        return self.lr

    def write_back(self):
        """Copy the trained values into the head's (and the backbone's) state dict (checkpoints,
        `state_dict()`)."""
        head = self.head
        for n, v in self.params.items():
            dst = self.backbone._params[n[len("backbone."):]] if n.startswith("backbone.") \
                else head._params[n]
            dst.copy_(v.to(dst.device))
        head._packed_version = head._weights_version()     # the packed device weights ARE these values
        if self.backbone is not None and hasattr(self.backbone, "_weights_version"):
            self.backbone._packed_version = self.backbone._weights_version()

    # ---------------------------------------------------------------- the state of a run
    # which of torch's DEFAULT generators `step()` draws from ("host", "device"); a subclass whose
    # loss draws its points with `torch.rand` names them here, and they travel with the state
    DEFAULT_GENERATORS = ()

    def _segment_index(self):
        return {n: i for i, n in enumerate(self.layout)}

    def _loss_buffers(self):
        """The loss's persistent buffers as host tensors, under the names its own `state_dict()`
        uses (SeesawLoss's `cum_samples` of `CrossHead2Loss` / `CrossHeadBBoxLoss`; read back
        from the device where the device copy is the live one).  The other heads' losses keep
        nothing between steps."""
        loss = getattr(self.head, "_loss", None)
        if loss is None or not hasattr(loss, "state_dict"):
            return OrderedDict()
        return OrderedDict((k, v.detach().cpu().clone()) for k, v in loss.state_dict().items())

    def state_dict(self):
        """Everything of a training run that the model's state dict does not hold, as host
        tensors and plain Python containers (loads under `torch.load(weights_only=True)`):

        "optimizer": the layout of `torch.optim.AdamW.state_dict()` -- ONE param group per trained
        parameter, in the order of `self.names` (mmcv's `DefaultOptimizerConstructor` makes one
        group per parameter when a `paramwise_cfg` is given: restated from memory, UNPINNED like
        the multiplier rule), each with `lr` (the scheduled rate x the segment's multiplier),
        `initial_lr`, `weight_decay`, `betas`, `eps`, `amsgrad=False` and `params=[i]`;
        `state[i] = {"step", "exp_avg", "exp_avg_sq"}` in the parameter's own shape; beside them
        `"param_names"`, so that a reader can map the entries by name.  Frozen layout names
        (multipliers 0) are not in it, as they are not in `params`.  (`step` is this trainer's
        host counter: it advances on a step whose guarded update was skipped on the device too.)

        "trainer": the class name, `steps`, `lr`, `base_lr`, the dropout's seed and subsequence,
        the `deterministic` / `device_targets` flags, the state of every generator `step()` draws
        from as uint8 tensors ("drop_path": the host generator of `_drop_path_keep`;
        "device_default" / "host_default": torch's default generators where the class's
        `DEFAULT_GENERATORS` names them) and "loss", the loss's persistent buffers.

        The dropout masks (csrc/dropout.hip) and the point draws of the segmentation and triplet
        losses are functions of (seed, rank, step, site): restoring `steps` restores them, nothing
        of theirs is stored (tests/test_runner_gpu.py resumes a dropout run bit for bit)."""
        seg = self._segment_index()
        lrs, wds = self.seg_lr.cpu().tolist(), self.seg_wd.cpu().tolist()
        base_lr = getattr(self, "base_lr", self.lr)
        groups, state = [], {}
        for i, n in enumerate(self.names):
            o, shape, k = self.layout[n]
            s = seg[n]
            groups.append(dict(lr=self.lr * lrs[s], initial_lr=base_lr * lrs[s],
                               weight_decay=self.wd * wds[s],
                               betas=(float(self.betas[0]), float(self.betas[1])),
                               eps=float(self.eps), amsgrad=False, params=[i]))
            state[i] = dict(step=torch.tensor(float(self.steps)),
                            exp_avg=self.flat_m[o:o + k].view(shape).cpu().clone(),
                            exp_avg_sq=self.flat_v[o:o + k].view(shape).cpu().clone())
        gens = OrderedDict()
        if hasattr(self, "_gen"):
            gens["drop_path"] = self._gen.get_state().clone()
        if "host" in self.DEFAULT_GENERATORS:
            gens["host_default"] = torch.get_rng_state().clone()
        if "device" in self.DEFAULT_GENERATORS:
            gens["device_default"] = torch.cuda.get_rng_state(self.dev).clone()
        trainer = {"class": type(self).__name__, "steps": int(self.steps), "lr": float(self.lr),
                   "base_lr": float(base_lr), "seed": int(getattr(self, "seed", 0)),
                   "subseq": int(getattr(self, "subseq", 0)),
                   "deterministic": bool(getattr(self, "deterministic", False)),
                   "device_targets": bool(getattr(self, "device_targets", False)),
                   "generators": gens, "loss": self._loss_buffers()}
        return {"optimizer": {"state": state, "param_groups": groups,
                              "param_names": list(self.names)},
                "trainer": trainer}

    def load_state_dict(self, sd):
        """Restore what `state_dict()` saved: `flat_m` / `flat_v` through views of the same
        layout, the counters and rates, the generators and the loss buffers.  The PARAMETERS come
        from the model's state dict, which is loaded before the trainer is built (the trainer's
        constructor copies them into `flat_p`): this does not touch `flat_p`.  Raises `ValueError`
        naming the first mismatch (class, parameter names, shapes) before anything is written."""
        opt, tr = sd["optimizer"], sd["trainer"]
        if tr["class"] != type(self).__name__:
            raise ValueError("trainer state of a %s loaded into a %s"
                             % (tr["class"], type(self).__name__))
        names = list(opt["param_names"])
        if names != list(self.names):
            first = next((i for i, (a, b) in enumerate(zip(names, self.names)) if a != b),
                         min(len(names), len(self.names)))
            raise ValueError("parameter names differ at entry %d: the state has %r, the trainer %r "
                             "(%d against %d names)"
                             % (first, names[first] if first < len(names) else None,
                                self.names[first] if first < len(self.names) else None,
                                len(names), len(self.names)))
        for i, n in enumerate(self.names):
            shape = tuple(self.layout[n][1])
            for key in ("exp_avg", "exp_avg_sq"):
                got = tuple(opt["state"][i][key].shape)
                if got != shape:
                    raise ValueError("%s of %s has shape %s, the trainer's parameter %s"
                                     % (key, n, got, shape))
        for flag in ("deterministic", "device_targets"):
            if bool(tr.get(flag, False)) != bool(getattr(self, flag, False)):
                raise ValueError("the state was saved with %s=%s, this trainer has %s=%s"
                                 % (flag, tr.get(flag), flag, getattr(self, flag, False)))
        for i, n in enumerate(self.names):
            o, shape, k = self.layout[n]
            self.flat_m[o:o + k].view(shape).copy_(opt["state"][i]["exp_avg"].to(torch.float32))
            self.flat_v[o:o + k].view(shape).copy_(opt["state"][i]["exp_avg_sq"].to(torch.float32))
        self.steps = int(tr["steps"])
        self.lr, self.base_lr = float(tr["lr"]), float(tr["base_lr"])
        if hasattr(self, "seed"):
            self.seed = int(tr["seed"])
        if hasattr(self, "subseq"):
            self.subseq = int(tr["subseq"])
        gens = tr.get("generators", {})
        if "drop_path" in gens and hasattr(self, "_gen"):
            self._gen.set_state(gens["drop_path"].cpu())
        if "host_default" in gens:
            torch.set_rng_state(gens["host_default"].cpu())
        if "device_default" in gens:
            torch.cuda.set_rng_state(gens["device_default"].cpu(), self.dev)
        if tr.get("loss"):
            self.head.loss_object().load_state_dict(tr["loss"])

    @torch.no_grad()
    @hip.on_device
    def apply_gradients(self, guard=None):
        """Clip (global L2 norm over the whole flat gradient) + AdamW on `flat_grad`, then the
        refresh of the derived packs.  `guard`: a device int32 word; non-zero skips the update on
        the device (`steps` advances all the same)."""
        g = self.flat_grad
        pre = self.reducer.scale if self.reducer is not None else 1.0
        hip.grad_norm_clip(g, self.clip, self._scratch, pre=pre, max_norm=self.max_norm)
        self.steps += 1
        hip.adamw(self.flat_p, g, self.flat_m, self.flat_v, self.seg_off, self.seg_lr, self.seg_wd,
                  self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self.steps,
                  clip=self.clip, pre=pre, guard=guard)
        self._refresh_derived()


# ---------------------------------------------------------------- the derived packs, one by one
# (module: the head, or the backbone; w: its packed device weights; p: the trainer's `params`)
def refresh_self_attention(head, w, p, decoder, layers, slot):
    """Self-attention of `decoder`'s layers as one [V | Q | K] projection; `slot`: the
    self-attention's place in a layer's `attentions` (0 for a self-first decoder)."""
    for i in range(layers):
        a = "%s.layers.%d.attentions.%d.attn." % (decoder, i, slot)
        W, b = p[a + "in_proj_weight"], p[a + "in_proj_bias"]
        w[a + "vqk.weight"][:256].copy_(W[512:])
        w[a + "vqk.weight"][256:].copy_(W[:512])
        w[a + "vqk.bias"][:256].copy_(b[512:])
        w[a + "vqk.bias"][256:].copy_(b[:512])


def refresh_relation_cross_attention(head, w, p):
    """The relation decoder's cross-attention keys / values: [V | K]."""
    for i in range(head.num_rel_layers):
        a = "relation_decoder.layers.%d.attentions.0.attn." % i
        W, b = p[a + "in_proj_weight"], p[a + "in_proj_bias"]
        w[a + "vk.weight"][:256].copy_(W[512:])
        w[a + "vk.weight"][256:].copy_(W[256:512])
        w[a + "vk.bias"][:256].copy_(b[512:])
        w[a + "vk.bias"][256:].copy_(b[256:512])


MATRIX_LEARNER = "update_importance.conv_layers."
MATRIX_LEARNER_REPACKED = (MATRIX_LEARNER + "1.0.weight", MATRIX_LEARNER + "2.0.weight")


def refresh_matrix_learner(head, w, p):
    """ConvTiny's two packed layouts."""
    ml = MATRIX_LEARNER
    w[ml + "1.0.weight"].copy_(p[ml + "1.0.weight"].permute(0, 2, 3, 1).reshape(64, -1))
    w[ml + "2.0.weight"].copy_(p[ml + "2.0.weight"].reshape(64, 49).t())


def refresh_r0(head, w, p):
    """`rel_query_feat` repeated over the batch."""
    for c in head._consts.values():
        if "r0" in c:
            B = c["r0"].shape[0] // p["rel_query_feat.weight"].shape[0]
            c["r0"].view(B, -1, 256).copy_(p["rel_query_feat.weight"].unsqueeze(0).expand(B, -1, -1))


def refresh_q0(head, w, p):
    """The initial queries repeated over the batch, and their mask embedding."""
    for c in head._consts.values():
        if "q0" not in c:
            continue
        BQ = c["q0"].shape[0]
        B = BQ // p["query_feat.weight"].shape[0]
        c["q0"].view(B, -1, 256).copy_(p["query_feat.weight"].unsqueeze(0).expand(B, -1, -1))
        if c.get("me0") is not None:
            tmp = SimpleNamespace(B=B, cls=None, MP=None,
                                  **{n: torch.empty(BQ, 256, device=head.device)
                                     for n in ("qn", "m1", "m2", "me")})
            head._head_embed(c["q0"], tmp, False, False)
            c["me0"].copy_(tmp.me)


def refresh_key_positions(head, w, p):
    """The key position tables carry `level_embed`."""
    for shapes, ent in head._pe.items():
        for l, (h, wd) in enumerate(shapes):
            hip.sine_pe(ent[1][l], p["level_embed.weight"][l], h, wd)


def refresh_query_positions(head, w, p):
    """The query position tables carry `level_encoding`; `pos8` follows them."""
    for shapes, ent in head._pe.items():
        o = 0
        for l, (h, wd) in enumerate(shapes):
            hip.sine_pe(ent[0][o:o + h * wd], p["pixel_decoder.level_encoding.weight"][l], h, wd)
            o += h * wd
        ent[3].copy_(hip.pos8(ent[0]))


def refresh_encoder(head, w, p):
    """One [value_proj | sampling_offsets | attention_weights] projection per encoder layer, and
    the bf16-pipe GEMMs' operand splits."""
    for i in range(head.num_enc_layers):
        q = "pixel_decoder.encoder.layers.%d." % i
        a = q + "attentions.0."
        o = 0
        for n in ("value_proj", "sampling_offsets", "attention_weights"):
            r = p[a + n + ".weight"].shape[0]
            w[a + "voa.weight"][o:o + r].copy_(p[a + n + ".weight"])
            w[a + "voa.bias"][o:o + r].copy_(p[a + n + ".bias"])
            o += r
        for k in (a + "voa.weight", a + "output_proj.weight", q + "ffns.0.layers.0.0.weight",
                  q + "ffns.0.layers.1.weight"):
            hip.s3_split(w[k], w[k + ".s3"])


FPN_CONV = "pixel_decoder.output_convs.0.conv."


def refresh_fpn_conv(head, w, p):
    """The FPN branch's 3x3 convolution: two Winograd forms and the direct one
    ([co][(ky * 3 + kx) * 256 + ci])."""
    cw = p[FPN_CONV + "weight"]
    w[FPN_CONV + "winograd"].copy_(hip.winograd_weights(cw))
    w[FPN_CONV + "winograd4"].copy_(hip.winograd43_weights(cw))
    w[FPN_CONV + "weight"].copy_(cw.permute(0, 2, 3, 1).reshape(256, -1))


def refresh_resnet(backbone, w, p, tape):
    """Re-fold BatchNorm into the trained convolutions and rewrite the backbone's packed
    weights (channel-last rows, Winograd transforms, bf16-plane splits)."""
    for n, sc in tape.bn_scale64.items():
        conv = n[:-len(".weight")]
        # W' = W gamma / sqrt(var + eps), formed in double and rounded once like `_fold`
        cw = (p["backbone." + n].double() * sc.view(-1, 1, 1, 1)).float()
        co = cw.shape[0]
        w[conv + ".w"].copy_(cw.permute(0, 2, 3, 1).reshape(co, -1))
        if conv + ".wino" in w:
            w[conv + ".wino"].copy_(hip.winograd_weights(cw.contiguous()))
            w[conv + ".wino4"].copy_(hip.winograd43_weights(cw.contiguous()))
        if conv + ".w.s3" in w:
            hip.s3_split(w[conv + ".w"], w[conv + ".w.s3"])


def refresh_swin(backbone, w, p, tape):
    """The Swin backbone's packed weights of the trained stages, as `SwinTransformerHip._pack`
    derives them: the bias tables transposed to [heads][(2ws-1)^2], the block GEMMs' bf16-plane
    splits, the patch-merging norm and reduction weight in neighbour-major column order, the
    patch-embedding weight in the first 48 of its 64 columns."""
    for n in tape.layout:
        v = p.get("backbone." + n)
        if v is None:                          # (norm0 without a gradient: never moves)
            continue
        if n.endswith("relative_position_bias_table"):
            v = v.t()
        elif ".downsample." in n:              # nn.Unfold order c*4 + q -> q*C + c
            c = v.shape[-1] // 4
            v = v.reshape(*v.shape[:-1], c, 4).transpose(-1, -2).reshape(v.shape)
        if n == "patch_embed.projection.weight":
            w[n][:, :48].copy_(v.reshape(v.shape[0], 48))
        else:
            w[n].copy_(v)
        if n + ".s3" in w:
            hip.s3_split(w[n], w[n + ".s3"])
