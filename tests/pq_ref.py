"""Panoptic quality the slow way: a second, independent statement of the specification in
INTEGRATION.md 3a-2 (`np.unique` over the joint key of the two maps, dict loops, Python floats).
`pairnet_amd.evaluation.PanopticQuality.add_host` is pinned by it and shares no code with it."""
import numpy as np

VOID = -1          # the void "segment" of either map in the dict keys below


def image_record(pred, gt_id, segments, num_classes=133, offset=1000):
    """pred / gt_id: integer maps [H, W]; segments: rows (id, category, iscrowd).  Returns
    dict(tp, fp, fn: {category: count}, iou: {category: float}, void_absorbed, crowd_absorbed:
    unmatched predictions not counted as false positives, N: {(gt id | VOID, segment | VOID):
    pixels})."""
    pred = np.asarray(pred).astype(np.int64)
    gt_id = np.asarray(gt_id).astype(np.int64)
    assert pred.shape == gt_id.shape and pred.min() >= 0 and pred.max() < 2 ** 32
    info = {int(i): (int(c), bool(k)) for i, c, k in segments}
    keys, counts = np.unique(gt_id * 2 ** 32 + pred, return_counts=True)
    N, pcat = {}, {}
    for key, n in zip(keys.tolist(), counts.tolist()):
        g, value = key // 2 ** 32, key % 2 ** 32
        if g == 0 or g not in info:
            g = VOID
        s, c = value // offset, value % offset
        assert c <= num_classes and s < 256
        if c == num_classes:
            p = VOID
        else:
            p = s
            assert pcat.setdefault(p, c) == c
        N[(g, p)] = N.get((g, p), 0) + n
    area_g, area_p = {}, {}
    for (g, p), n in N.items():
        area_g[g] = area_g.get(g, 0) + n
        area_p[p] = area_p.get(p, 0) + n
    tp, fp, fn, iou = {}, {}, {}, {}
    matched_g, matched_p = set(), set()
    for g, p in sorted(N):                      # ascending ground-truth id
        if g == VOID or p == VOID:
            continue
        cat, crowd = info[g]
        if crowd or pcat[p] != cat:
            continue
        n = N[(g, p)]
        union = area_p[p] + area_g[g] - n - N.get((VOID, p), 0)
        if n / union > 0.5:
            assert g not in matched_g and p not in matched_p
            matched_g.add(g)
            matched_p.add(p)
            tp[cat] = tp.get(cat, 0) + 1
            iou[cat] = iou.get(cat, 0.0) + n / union
    for g in sorted(info):
        cat, crowd = info[g]
        if not crowd and g not in matched_g:
            fn[cat] = fn.get(cat, 0) + 1
    void_absorbed = crowd_absorbed = 0
    for p in sorted(pcat):
        if p in matched_p:
            continue
        void = N.get((VOID, p), 0)
        crowd = sum(n for (g, q), n in N.items()
                    if q == p and g != VOID and info[g][1] and info[g][0] == pcat[p])
        if (void + crowd) / area_p[p] > 0.5:
            if void / area_p[p] > 0.5:
                void_absorbed += 1
            else:
                crowd_absorbed += 1
            continue
        fp[pcat[p]] = fp.get(pcat[p], 0) + 1
    return dict(tp=tp, fp=fp, fn=fn, iou=iou, void_absorbed=void_absorbed,
                crowd_absorbed=crowd_absorbed, N=N)


def dense(rec, num_classes):
    """(ints [num_classes][3] int32, iou [num_classes] float64) of an `image_record`."""
    ints = np.zeros((num_classes, 3), np.int32)
    iou = np.zeros(num_classes, np.float64)
    for j, k in enumerate(("tp", "fp", "fn")):
        for c, n in rec[k].items():
            ints[c, j] = n
    for c, v in rec["iou"].items():
        iou[c] = v
    return ints, iou


def dense_table(rec, segments, G):
    """N [(G + 1)][257] int32 of an `image_record`: row 0 / column 256 void, rows in id order."""
    rows = {int(i): r + 1 for r, i in enumerate(sorted(int(s[0]) for s in segments))}
    out = np.zeros((G + 1, 257), np.int32)
    for (g, p), n in rec["N"].items():
        out[0 if g == VOID else rows[g], 256 if p == VOID else p] += n
    return out


def summarize(records, num_classes=133, num_things=80):
    """records: the `image_record`s in dataset order."""
    tp, fp, fn, iou = ([0] * num_classes for _ in range(4))
    iou = [0.0] * num_classes
    for r in records:
        for c in range(num_classes):
            tp[c] += r["tp"].get(c, 0)
            fp[c] += r["fp"].get(c, 0)
            fn[c] += r["fn"].get(c, 0)
            iou[c] += r["iou"].get(c, 0.0)
    per = {}
    for c in range(num_classes):
        if tp[c] + fp[c] + fn[c] > 0:
            den = tp[c] + 0.5 * fp[c] + 0.5 * fn[c]
            per[c] = (iou[c] / den, iou[c] / tp[c] if tp[c] else 0.0, tp[c] / den)
    out = dict(images=len(records), classwise=per, n={})
    for name, suffix, cats in (("all", "", range(num_classes)),
                               ("things", "_th", range(num_things)),
                               ("stuff", "_st", range(num_things, num_classes))):
        rows = [per[c] for c in cats if c in per]
        out["n"][name] = len(rows)
        for j, key in enumerate(("PQ", "SQ", "RQ")):
            total = 0.0
            for r in rows:
                total += r[j]
            out[key + suffix] = 100.0 * (total / len(rows)) if rows else 0.0
    return out
