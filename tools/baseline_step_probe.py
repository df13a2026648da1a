"""Times the masked key-split attention backward and the sibling head's training step (labnotes R24)
at B = 1 and the shapes of an 800 x 1333 image:

  attention   pn_mha_bwd_keysplit_masked_f32 beside pn_mha_bwd_f32 under the same bits, ALTERNATING
              calls in one process, Nq = 100 against the three memory levels (1 050, 4 200, 16 700
              keys), for two mask families: "random" (random operands, half the keys masked) and
              "head" (the bits, queries, keys and values a SEEDED head's own nine masked layers
              produce at 800 x 1333, three layers per level).  Nobody has measured a trained model's
              mask density; the seeded head's is printed and recorded per layer.  Each case also
              records both kernels' worst error against float64 autograd in the tests' row measure.
  step        one `BaselineTrainer.step` from the image (ResNet-50 stages 2-4 + the whole head), the
              head tape's `masked_keysplit_min_keys` off (None) and on, alternating on ONE trainer
              (whose parameters move from call to call), with the `grad_norm` of the SAME first
              step under both settings (parameters and moments put back between the two).

HIP events around each call, 3 warm-up calls, median with min-max of `--iters` calls, `--repeats`
times (the R20.4 / R23.4 protocol).  `default_min_keys`: the smallest level at and above which the
new kernel was faster in every repeat for both families (every layer of the level), or null.

    python tools/baseline_step_probe.py [--iters 20] [--repeats 3] [--out profiles/baseline_step.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from fpn_grad_probe import timed_alternating  # noqa: E402

DEV = "cuda:0"
LEVELS = (1050, 4200, 16700)
SCALE = 32 ** -0.5


def pair(hip, q, k, v, do, bits, rowall, B, Nq, Nk):
    """(new, old, outs): the two kernels on the same operands and bits."""
    outs = [[torch.empty(B * n, 256, device=DEV) for n in (Nq, Nk, Nk)] for _ in range(2)]
    ks_scr = torch.empty(hip.mha_bwd_keysplit_scratch_floats(B, Nq, Nk), device=DEV)
    scr = torch.empty(hip.mha_bwd_scratch_floats(B, Nq, Nk), device=DEV)
    new = lambda: hip.mha_bwd_keysplit(q, k, v, do, *outs[0], ks_scr, B, Nq, Nk, SCALE,
                                       bits=bits, rowall=rowall)
    old = lambda: hip.mha_bwd(q, k, v, do, *outs[1], scr, B, Nq, Nk, SCALE, bits=bits, rowall=rowall)
    return new, old, outs


def unpack(bits, rowall, Nq, Nk):
    """The boolean mask [Nq, Nk] as the kernels see it (a rowall row masks nothing)."""
    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    m = ((bits.view(Nq, -1, 1) >> sh) & 1).reshape(Nq, -1)[:, :Nk].bool()
    return m & ~rowall.bool().view(Nq, 1)


def worst_ratios(outs, refs):
    """Worst |err| / (2^-24 max |ref row|) of dq / dk / dv against float64 (the tests' row bound)."""
    out = []
    for a, r in zip(outs, refs):
        r = r.to(a.device).double()
        mag = r.abs().amax(-1, keepdim=True).clamp_min(2.0 ** -126)
        out.append(float(((a.double() - r).abs() / (2.0 ** -24 * mag)).max()))
    return dict(zip(("dq", "dk", "dv"), out))


def random_case(hip, Nk, Nq=100, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + Nk)
    r = lambda n: torch.randn(n, 256, generator=g, device=DEV)
    q, k, v, do = r(Nq), r(Nk), r(Nk), r(Nq)
    lg = torch.rand(Nq, Nk, generator=g, device=DEV) - 0.5
    bits = torch.empty(Nq, (Nk + 31) // 32, dtype=torch.int32, device=DEV)
    rowall = torch.empty(Nq, dtype=torch.int32, device=DEV)
    hip.mask_pack(lg, bits, rowall, Nq, Nk)
    return q, k, v, do, bits, rowall


def seeded_head(H, W):
    from helpers import baseline_cfg, oracle_baseline_head
    from pairnet_amd import CrossHeadBaseline
    _, sd, _ = oracle_baseline_head(1234)
    head = CrossHeadBaseline(**baseline_cfg())
    head.load_state_dict(sd)
    head.to(DEV)
    return head


def attention(args, res, hip):
    from oracle import seeded
    from pairnet_amd import SegmenterHeadGrad
    from test_grad_kernels_gpu import _mha_ref
    H, W = 800, 1333
    head = seeded_head(H, W)
    head.return_all_layers = True
    head.forward([f.to(DEV) for f in seeded.seeded_feats(99, 1, H, W)],
                 [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4)])
    pl = head._last_plan
    assert tuple(pl.N) == LEVELS, pl.N
    tape = SegmenterHeadGrad(head)
    tape.forward_from_plan(pl)
    g = torch.Generator(device=DEV).manual_seed(7)
    cases = {}
    for Nk in LEVELS:
        cases[("random", Nk, None)] = random_case(hip, Nk)
    for i, s in enumerate(tape.dt["layers"]):
        Nk = pl.N[s["level"]]
        do = torch.randn(100, 256, generator=g, device=DEV)
        cases[("head", Nk, i)] = (s["Qc"], s["K"], s["V"], do, s["bits"], s["rowall"])
    table = {}
    for key, (q, k, v, do, bits, rowall) in cases.items():
        fam, Nk, layer = key
        new, old, outs = pair(hip, q, k, v, do, bits, rowall, 1, 100, Nk)
        new(), old()
        torch.cuda.synchronize()
        m = unpack(bits, rowall, 100, Nk)
        d, ra = float(m.float().mean()), int(rowall.sum())
        with torch.enable_grad():
            refs = _mha_ref(q, k, v, do, 1, 100, Nk, SCALE, (~m).view(1, 100, Nk))
        name = "%s/%d" % (fam, Nk) + ("" if layer is None else "/layer%d" % layer)
        table[name] = dict(family=fam, keys=Nk, layer=layer, masked_share=d, rowall_rows=ra,
                           worst_ratio_float64=dict(keysplit_masked=worst_ratios(outs[0], refs),
                                                    mha_bwd=worst_ratios(outs[1], refs)),
                           max_abs_difference=dict(zip(("dq", "dk", "dv"),
                                                       [float((a - b).abs().max()) for a, b in zip(*outs)])),
                           max_abs=dict(zip(("dq", "dk", "dv"), [float(b.abs().max()) for b in outs[1]])),
                           runs=[], fns=(new, old))
        print("%-22s masked share %.3f, %d rowall rows; worst ratio against float64 %s"
              % (name, d, ra, {kk: {a: round(b, 1) for a, b in vv.items()}
                               for kk, vv in table[name]["worst_ratio_float64"].items()}), flush=True)
    for rep in range(args.repeats):
        for name, e in table.items():
            a, b = timed_alternating(*e["fns"], args.iters)
            e["runs"].append(dict(keysplit_masked=a, mha_bwd=b))
            print("repeat %d %-22s keysplit_masked %.3f ms (%.3f-%.3f), mha_bwd %.3f ms (%.3f-%.3f), "
                  "ratio %.2f" % (rep, name, a["median"], a["min"], a["max"], b["median"], b["min"],
                                  b["max"], b["median"] / a["median"]), flush=True)
    faster = {}
    for name, e in table.items():
        del e["fns"]
        e["mha_bwd_over_keysplit_masked"] = [r["mha_bwd"]["median"] / r["keysplit_masked"]["median"]
                                             for r in e["runs"]]
        faster.setdefault(e["keys"], []).append(min(e["mha_bwd_over_keysplit_masked"]) > 1.0)
    res["attention"] = table
    res["level_faster_in_every_repeat_for_both_families"] = {str(n): all(faster[n]) for n in LEVELS}
    default = None
    for n in reversed(LEVELS):           # the smallest level AT AND ABOVE which it holds
        if not all(faster[n]):
            break
        default = n
    res["default_min_keys"] = default
    print("default masked_keysplit_min_keys:", default, flush=True)
    del tape, head
    torch.cuda.empty_cache()
    return default


def step(args, res, default):
    from pairnet_amd import BaselineTrainer, ResNet50Hip
    H, W, n_obj = 800, 1333, 12
    head = seeded_head(H, W)
    bb = ResNet50Hip().to(DEV)
    g = torch.Generator().manual_seed(11)
    img = torch.randn(1, 3, H, W, generator=g).to(DEV)
    metas = [dict(img_shape=(H, W, 3), scale_factor=[1.0] * 4, batch_input_shape=(H, W))]
    gt_labels = [torch.randint(0, 133, (n_obj,), generator=g)]
    gt_masks = [(torch.rand(n_obj, H // 2, W // 2, generator=g) > 0.6).to(torch.uint8).to(DEV)]
    pairs = torch.randperm(n_obj * n_obj, generator=g)[:8]
    gt_rels = [torch.stack([pairs // n_obj, pairs % n_obj,
                            torch.randint(1, 57, (8,), generator=g)], 1)]
    gt_rels = [r[r[:, 0] != r[:, 1]] for r in gt_rels]
    tr = BaselineTrainer(head, backbone=bb, masked_keysplit_min_keys=None)
    on_value = default if default is not None else LEVELS[0]
    # the same first step under both settings: parameters, moments and step count put back between
    norms, state = {}, (tr.flat_p, tr.flat_m, tr.flat_v)
    snap = [t.clone() for t in state]
    for name, mk in (("off", None), ("on", on_value)):
        for t, s in zip(state, snap):
            t.copy_(s)
        tr.steps = 0
        tr._refresh_derived()
        tr.tape.masked_keysplit_min_keys = mk
        norms[name] = float(tr.step(img, metas, gt_rels, gt_labels, gt_masks)["grad_norm"])

    def variant(mk):
        def run():
            tr.tape.masked_keysplit_min_keys = mk
            tr.step(img, metas, gt_rels, gt_labels, gt_masks)
        return run

    off, on = variant(None), variant(on_value)
    res["step"] = dict(shape=dict(B=1, H=H, W=W, objects=n_obj, relations=int(gt_rels[0].shape[0])),
                       on_min_keys=on_value, parameters=int(tr.n), runs=[])
    for rep in range(args.repeats):
        a, b = timed_alternating(off, on, args.iters)
        res["step"]["runs"].append(dict(off=a, on=b))
        print("repeat %d step: off %.2f ms (%.2f-%.2f), on (min_keys %d) %.2f ms (%.2f-%.2f), ratio %.3f"
              % (rep, a["median"], a["min"], a["max"], on_value, b["median"], b["min"], b["max"],
                 a["median"] / b["median"]), flush=True)
    torch.cuda.synchronize()
    res["step"]["first_grad_norm"] = norms
    res["step"]["off_over_on"] = [r["off"]["median"] / r["on"]["median"] for r in res["step"]["runs"]]
    res["step"]["assign_status_last"] = int(tr._guard[0])
    print("first grad_norm:", res["step"]["first_grad_norm"], "last status",
          res["step"]["assign_status_last"], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--attention-only", action="store_true")
    args = ap.parse_args()
    from pairnet_amd import hip
    res = dict(chunk=hip.MHA_KEYSPLIT_CHUNK)
    with torch.no_grad():
        default = attention(args, res, hip)
        if not args.attention_only:
            step(args, res, default)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
