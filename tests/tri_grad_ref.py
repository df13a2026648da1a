"""Float64 statements for the backward of `PSGTrHead2` behind its logits (plain torch; shares no code
with the package):

  * `heads` / `functional`: the two-"layer" head chain of psgtr_head2.py:288-444 as the reference
    ends up wiring it (sic) -- `sub_seg` = obj_mask_embed(post_norm(q_last)) . MF, `obj_seg` =
    obj_mask_embed(post_norm(query_feat)) . MF, the three class heads on post_norm(q_last) -- and the
    linear functional whose gradient the tape's `backward` computes from the loss's compact
    gradients;
  * `kernel_*`: `pn_triplet_heads_bwd_f32`'s two results (csrc/tri_grad.hip), the sums of absolute
    products they are bounded against, the cases and the bound.

The bound, in the project's form: |got - ref64| <= c * 2^-24 * mag + FLT_MIN with c = the contraction
length + a, where the length is 2 (C + 1) + (Cr + 1) + 1 for dqn (one chain over the columns of the
three heads, + the preloaded value) and N for dW / db, and a = max(4, twice the worst ratio
|torch fp32 - ref64| / (2^-24 * mag) of torch's own fp32 result on that case).  Nothing in it comes
from the kernel's measured error."""
import torch

FLT_MIN = 1.17549435e-38
EPS = 2.0 ** -24

HEAD_PARAMS = ["%s_cls_embed.%s" % (h, n) for h in ("sub", "obj", "rel") for n in ("weight", "bias")] + \
    ["obj_mask_embed.%d.%s" % (j, n) for j in (0, 2, 4) for n in ("weight", "bias")] + \
    ["transformer_decoder.post_norm.weight", "transformer_decoder.post_norm.bias"]
UNREACHED = ["%s.%d.%s" % (m, j, n) for m in ("mask_embed", "sub_mask_embed") for j in (0, 2, 4)
             for n in ("weight", "bias")]


# ------------------------------------------------------------------------- the head chain
def _post_norm(x, p):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * p["transformer_decoder.post_norm.weight"] + \
        p["transformer_decoder.post_norm.bias"]


def _mlp3(x, p, name):
    for j in (0, 2, 4):
        x = x @ p["%s.%d.weight" % (name, j)].t() + p["%s.%d.bias" % (name, j)]
        if j < 4:
            x = torch.relu(x)
    return x


def heads(q_last, query_feat, MF, p):
    """q_last [B, Q, 256] (the last decoder layer's output before post_norm), query_feat [Q, 256],
    MF [B, P, 256], p: {reference parameter name: tensor} -> sub, obj [B, Q, C + 1], rel
    [B, Q, Cr + 1], sub_seg, obj_seg [B, Q, P]."""
    B = q_last.shape[0]
    x = _post_norm(q_last, p)
    lin = lambda name: x @ p[name + ".weight"].t() + p[name + ".bias"]
    sub, obj, rel = lin("sub_cls_embed"), lin("obj_cls_embed"), lin("rel_cls_embed")
    sub_seg = torch.einsum("bqc,bpc->bqp", _mlp3(x, p, "obj_mask_embed"), MF)          # sic
    x0 = _post_norm(query_feat.unsqueeze(0).expand(B, -1, -1), p)
    obj_seg = torch.einsum("bqc,bpc->bqp", _mlp3(x0, p, "obj_mask_embed"), MF)         # stale
    return sub, obj, rel, sub_seg, obj_seg


def functional(out, g_sub, g_obj, g_rel, G_sub, G_obj, rows):
    """F = sum sub . g_sub + sum obj . g_obj + sum rel . g_rel + sum over m with rows[m] >= 0 of
    sub_seg[rows[m]] . G_sub[m] + obj_seg[rows[m]] . G_obj[m]; rows index the B * Q query rows, a
    row < 0 (a failed image) is skipped and its G rows are not read."""
    sub, obj, rel, sub_seg, obj_seg = out
    F = (sub * g_sub.reshape(sub.shape)).sum() + (obj * g_obj.reshape(obj.shape)).sum() + \
        (rel * g_rel.reshape(rel.shape)).sum()
    P = sub_seg.shape[-1]
    s2, o2 = sub_seg.reshape(-1, P), obj_seg.reshape(-1, P)
    for m, r in enumerate(rows.tolist()):
        if r >= 0:
            F = F + (s2[r] * G_sub[m].reshape(P)).sum() + (o2[r] * G_obj[m].reshape(P)).sum()
    return F


# ------------------------------------------------------------------------- the kernel
#              N   C + 1  Cr + 1
CASES = {"tiny": dict(N=6, C1=5, Cr1=3),                        # every tile ragged
         "one-past": dict(N=33, C1=134, Cr1=57),                # one row past a 32-row tile
         "production": dict(N=200, C1=134, Cr1=57),             # B 2, Q 100, 133 classes, 56 relations
         "zero-rel": dict(N=70, C1=134, Cr1=57, zero_rel=True),  # drel == 0, dsub with a zero row
         "add": dict(N=70, C1=134, Cr1=57, add=True)}           # dqn preloaded
_cache = {}


def kernel_case(name):
    """fp32 host operands of a case: dsub, dobj [N, C1], drel [N, Cr1], qn [N, 256], Wsub, Wobj
    [C1, 256], Wrel [Cr1, 256], pre [N, 256] (what dqn holds before the call), add."""
    if ("case", name) not in _cache:
        c = CASES[name]
        N, C1, Cr1 = c["N"], c["C1"], c["Cr1"]
        g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
        r = lambda *s: torch.randn(*s, generator=g)
        case = dict(dsub=r(N, C1), dobj=r(N, C1), drel=r(N, Cr1), qn=r(N, 256),
                    Wsub=r(C1, 256) * 0.06, Wobj=r(C1, 256) * 0.06, Wrel=r(Cr1, 256) * 0.06,
                    pre=r(N, 256), add=bool(c.get("add", False)), N=N, C1=C1, Cr1=Cr1)
        if c.get("zero_rel"):
            case["drel"].zero_()
            case["dsub"][N // 2].zero_()
        _cache["case", name] = case
    return _cache["case", name]


OUTPUTS = ("dqn", "dWsub", "dbsub", "dWobj", "dbobj", "dWrel", "dbrel")


def _products(case, dtype, absolute=False):
    f = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    d = {h: f(case["d" + h]) for h in ("sub", "obj", "rel")}
    W = {h: f(case["W" + h]) for h in ("sub", "obj", "rel")}
    qn = f(case["qn"])
    out = {"dqn": d["sub"] @ W["sub"] + d["obj"] @ W["obj"] + d["rel"] @ W["rel"]}
    if case["add"]:
        out["dqn"] = f(case["pre"]) + out["dqn"]
    for h in ("sub", "obj", "rel"):
        out["dW" + h] = d[h].t() @ qn
        out["db" + h] = d[h].sum(0)
    return out


def kernel_ref64(case):
    return _products(case, torch.float64)


def kernel_mag64(case):
    """The float64 sums of absolute products (and of |pre| where it is added)."""
    return _products(case, torch.float64, absolute=True)


def kernel_torch32(case):
    """torch's own fp32 result of the same expressions on the host."""
    return _products(case, torch.float32)


def contraction(case, key):
    return 2 * case["C1"] + case["Cr1"] + 1 if key == "dqn" else case["N"]


def ratios(got, ref, mag):
    """Elementwise |got - ref64| / (2^-24 * mag), 0 where both the error and mag are 0."""
    err = (got.double() - ref).abs()
    den = EPS * mag
    return torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, err / FLT_MIN, err))


def slack(name):
    """a of a case: max(4, twice torch-fp32's worst ratio over the case's seven outputs)."""
    if ("a", name) not in _cache:
        case = kernel_case(name)
        ref, mag, t32 = kernel_ref64(case), kernel_mag64(case), kernel_torch32(case)
        worst = max(float(ratios(t32[k], ref[k], mag[k]).max()) for k in OUTPUTS)
        _cache["a", name] = max(4.0, 2.0 * worst)
    return _cache["a", name]


def bound(name, key):
    """The allowed |got - ref64| of output `key` of case `name`, elementwise."""
    case = kernel_case(name)
    c = contraction(case, key) + slack(name)
    return c * EPS * kernel_mag64(case)[key] + FLT_MIN


def within(name, key, got):
    """-> (ok, worst ratio |err| / (2^-24 mag), its share of c)."""
    case = kernel_case(name)
    ref, mag = kernel_ref64(case)[key], kernel_mag64(case)[key]
    err = (got.double().cpu() - ref).abs()
    ok = bool((err <= bound(name, key)).all())
    worst = float(ratios(got.cpu(), ref, mag).max())
    return ok, worst, worst / (contraction(case, key) + slack(name))
