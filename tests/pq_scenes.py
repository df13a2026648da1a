"""Scenes for the panoptic-quality tests (CPU and GPU): a random ground truth and a prediction
DERIVED from it, so that IoU > 0.5 pairs exist (two independent random maps never reach 0.5 and
would pass a broken matcher)."""
import numpy as np

NC, OFFSET = 133, 1000
CATS = (0, 3, 79, 80, 100, 132)     # things and stuff, both ends of either range


def rgb_of(gt_id):
    g = np.asarray(gt_id).astype(np.int64)
    return np.stack([g & 255, (g >> 8) & 255, (g >> 16) & 255], -1).astype(np.uint8)


def voronoi(rng, H, W, R):
    """[H, W] labels 0..R-1: the nearest of R random seed pixels."""
    seeds = rng.choice(H * W, R, replace=False)
    yy, xx = np.mgrid[0:H, 0:W]
    best = np.full((H, W), np.iinfo(np.int64).max)
    lab = np.zeros((H, W), np.int64)
    for r, s in enumerate(seeds):
        d = (yy - s // W) ** 2 + (xx - s % W) ** 2
        m = d < best
        best[m], lab[m] = d[m], r
    return lab, seeds


def make_scene(seed, H, W, n_gt, perturb=True, split=1, ids=None):
    """Regions 0..n_gt-1 are the listed segments (as far as the map has pixels for them; the rest
    of the table has no pixel), region n_gt is void (id 0), region n_gt + 1 carries an id that
    is not in the table.  Region 1 is a crowd.  The prediction covers region r with segment
    (255 - r) % 256 of the region's category -- segment indices 255 and 0 occur -- shifted by
    1-3 pixels along one axis; then two segments are merged, `split` are split, one is relabelled, one is
    dropped (void class).  Returns dict(pred, gt_id, rgb, segments (n_gt, 3) sorted by id)."""
    rng = np.random.default_rng(seed)
    R = max(1, min(n_gt + 2, H * W))
    lab, seeds = voronoi(rng, H, W, R)
    if ids is None:
        ids = np.sort(rng.choice((1 << 24) - 1, n_gt + 1, replace=False) + 1)
    ids = np.asarray(ids, np.int64)
    cats = rng.choice(CATS, n_gt + 2)
    crowd = np.zeros(n_gt, np.int64)
    if n_gt > 3:
        crowd[1] = 1
    idmap = np.zeros(R, np.int64)
    for r in range(R):
        idmap[r] = ids[r] if r < n_gt else (0 if r == n_gt else ids[n_gt])
    gt_id = idmap[lab]
    seg_of = np.array([(255 - r) % 256 if r < 256 else -1 for r in range(R)])
    seg_cat = {int(seg_of[r]): int(cats[r]) for r in range(R) if seg_of[r] >= 0}
    plab = lab
    if perturb and H * W > 1:
        axis = int(rng.integers(0, 2)) if min(H, W) > 1 else int(W > 1)
        plab = np.roll(lab, int(rng.integers(1, 4)), axis)
    pseg = seg_of[plab]
    if perturb and n_gt >= 8 and R == n_gt + 2:
        pick = [int(r) for r in rng.permutation(np.arange(2, min(n_gt, 256)))]
        a, b, rel, drop = pick[:4]
        pseg[plab == a] = seg_of[b]                               # merged into b's segment
        free = [s for s in range(256) if s not in seg_cat]
        for r in pick[4:4 + split]:                               # split along its seed column
            if not free:
                break
            s = free.pop()
            seg_cat[s] = seg_cat[int(seg_of[r])]
            xx = np.broadcast_to(np.arange(W), (H, W))
            pseg[(plab == r) & (xx > seeds[r] % W)] = s
        seg_cat[int(seg_of[rel])] = int(CATS[(CATS.index(seg_cat[int(seg_of[rel])]) + 1)
                                              % len(CATS)])       # another category
        pseg[plab == drop] = -1
    cat_of = np.full(257, NC, np.int64)
    for s, c in seg_cat.items():
        cat_of[s] = c
    pred = np.where(pseg >= 0, pseg * OFFSET + cat_of[pseg], NC).astype(np.int64)
    segments = np.stack([ids[:n_gt], cats[:n_gt], crowd], 1).astype(np.int64)
    return dict(pred=pred, gt_id=gt_id, rgb=rgb_of(gt_id), segments=segments)
