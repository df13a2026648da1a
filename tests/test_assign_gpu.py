"""GPU: `pn_lsa_f32` (csrc/assign.hip) against `scipy.optimize.linear_sum_assignment` -- row_ind and
col_ind EXACTLY equal, ties included -- at the sizes where lane striding (63 / 64 / 65 / 128 / 129),
the transpose (cols < rows), the wave argmin and the two cost paths (staged in LDS / read from
memory) can go wrong; its status word on the inputs scipy raises on; and `pn_loss_targets` against
the numpy lines of pair-net_amd/losses.py on hand-built assignments."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import lsa_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("random", "ints", "dup")
SHAPES = [(1, 1), (1, 5), (5, 1), (7, 7), (100, 5), (100, 37), (37, 100), (100, 100)] + \
    [s for L in (63, 64, 65, 128, 129) for s in ((L, 9), (9, L))] + \
    [(200, 60), (12, 1024),
     (24, 1024),          # 24576 entries: the largest matrix that is staged in LDS
     (30, 1024)]          # 30720 entries: above the staging limit, read from memory


def solve(costs, max_cells=None):
    """One pn_lsa_f32 launch over `costs` (list of fp32 matrices) -> [(row_ind, col_ind, status)]."""
    from pairnet_amd import hip
    table, c_off, o_off = [], 0, 0
    for c in costs:
        table.append([c_off, c.shape[0], c.shape[1], o_off])
        c_off += c.size
        o_off += min(c.shape)
    flat = torch.from_numpy(np.concatenate([np.ascontiguousarray(c, np.float32).ravel() for c in costs]))
    # (guard words around the outputs: nothing may be written outside a problem's own entries)
    rows = torch.full((o_off + 8,), -7, dtype=torch.int32, device=DEV)
    cols = torch.full((o_off + 8,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((len(costs),), -7, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        hip.lsa(flat.to(DEV), torch.tensor(table, dtype=torch.int64, device=DEV), rows[:o_off],
                cols[:o_off], status,
                max_cells=max(c.size for c in costs) if max_cells is None else max_cells)
    rows, cols, status = rows.cpu().numpy(), cols.cpu().numpy(), status.cpu().numpy()
    assert (rows[o_off:] == -7).all() and (cols[o_off:] == -7).all()
    return [(rows[t[3]:t[3] + min(t[1], t[2])], cols[t[3]:t[3] + min(t[1], t[2])], int(st))
            for t, st in zip(table, status)]


def check(cost, got):
    want_r, want_c = linear_sum_assignment(cost.astype(np.float64))
    r, c, st = got
    assert st == 0, (cost.shape, st)
    assert np.array_equal(r, want_r) and np.array_equal(c, want_c), (cost.shape, r, c, want_r, want_c)
    # the same pairs: the same total in float64, exactly
    assert cost.astype(np.float64)[r, c].sum() == cost.astype(np.float64)[want_r, want_c].sum()


@pytest.mark.parametrize("kind", KINDS)
def test_single_problem_launches_equal_scipy(kind):
    rng = np.random.default_rng(10 + KINDS.index(kind))
    for rows, cols in SHAPES:
        cost = lsa_ref.problems(kind, rows, cols, rng)
        check(cost, solve([cost])[0])


@pytest.mark.parametrize("kind", KINDS)
def test_costs_read_from_memory_equal_scipy(kind):
    """max_cells = 0: no LDS staging, the other cost path of the kernel, both orientations."""
    rng = np.random.default_rng(20 + KINDS.index(kind))
    for rows, cols in ((100, 5), (37, 100), (65, 9), (9, 129), (100, 100)):
        cost = lsa_ref.problems(kind, rows, cols, rng)
        check(cost, solve([cost], max_cells=0)[0])


def test_one_launch_with_eight_mixed_problems():
    rng = np.random.default_rng(30)
    shapes = [(100, 5), (100, 3), (1, 1), (37, 100), (100, 100), (9, 65), (200, 60), (5, 1)]
    costs = [lsa_ref.problems(KINDS[i % 3], r, c, rng) for i, (r, c) in enumerate(shapes)]
    for cost, got in zip(costs, solve(costs)):
        check(cost, got)


def test_the_fixture_s_tie_is_broken_like_scipy():
    """Two ground-truth triplets of one (subject class, object class) pair give bit-identical cost
    columns (r_cls_cost's weight is 0): which relation query gets which decides its label."""
    rng = np.random.default_rng(31)
    for T in (2, 5, 12):
        c = rng.standard_normal((100, T)).astype(np.float32)
        c[:, T - 1] = c[:, 0]
        check(c, solve([c])[0])
        check(np.ascontiguousarray(c.T), solve([np.ascontiguousarray(c.T)])[0])


def test_status_word_on_what_scipy_raises_on():
    rng = np.random.default_rng(32)
    good = [lsa_ref.problems("dup", 100, 7, rng), lsa_ref.problems("random", 9, 64, rng)]
    nan = lsa_ref.problems("random", 100, 5, rng)
    nan[17, 3] = np.nan
    ninf = lsa_ref.problems("random", 6, 40, rng)
    ninf[5, 39] = -np.inf
    infrow = lsa_ref.problems("random", 5, 9, rng)
    infrow[2, :] = np.inf
    infcol = lsa_ref.problems("random", 100, 4, rng)      # (transposed: a row of the solver's matrix)
    infcol[:, 1] = np.inf
    one_inf = lsa_ref.problems("random", 100, 6, rng)     # a single +inf entry is ordinary data
    one_inf[3, 2] = np.inf
    for bad in (nan, ninf, infrow, infcol):
        with pytest.raises(ValueError):
            linear_sum_assignment(bad)
    costs = [good[0], nan, ninf, good[1], infrow, infcol, one_inf]
    got = solve(costs)
    assert [g[2] for g in got] == [0, 1, 1, 0, 2, 2, 0]
    for i in (1, 2, 4, 5):
        assert (got[i][0] == -1).all() and (got[i][1] == -1).all() and len(got[i][0]) == min(costs[i].shape)
    for i in (0, 3, 6):
        check(costs[i], got[i])


def test_descriptor_outside_the_operands_is_reported_not_followed():
    from pairnet_amd import hip
    cost = torch.zeros(20, device=DEV)
    table = torch.tensor([[0, 4, 5, 0], [0, 5, 5, 0], [0, 4, 5, 2], [0, 2000, 1, 0], [-4, 2, 2, 0]],
                         dtype=torch.int64, device=DEV)
    rows = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    cols = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((5,), -7, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        hip.lsa(cost, table, rows, cols, status, max_cells=20)
    assert status.cpu().tolist() == [0, 3, 3, 3, 3]
    assert rows.cpu().tolist() == [0, 1, 2, 3]


# ---- pn_loss_targets ---------------------------------------------------------------------------
def numpy_targets(Q, R, gl, gt_rels, rows, cols, rows2, cols2):
    """pair-net_amd/losses.py `_targets_single` from the two assignments on (the host path)."""
    query_of_gt = np.ones(len(gl), dtype=np.int64)
    order = np.argsort(rows)
    query_of_gt[cols[order]] = rows[order]
    gt_rel = gt_rels[:, 2] - 1
    gt_sub_cls, gt_obj_cls = gl[gt_rels[:, 0]], gl[gt_rels[:, 1]]
    importance = np.zeros((Q, Q), dtype=np.float32)
    importance[query_of_gt[gt_rels[:, 0]], query_of_gt[gt_rels[:, 1]]] = 1.0
    r_labels = np.full(R, -1, dtype=np.int64)
    sub_ids, obj_ids = r_labels.copy(), r_labels.copy()
    r_labels[rows2], sub_ids[rows2], obj_ids[rows2] = gt_rel[cols2], gt_sub_cls[cols2], gt_obj_cls[cols2]
    return r_labels, sub_ids, obj_ids, importance


Q_, R_, C_ = 6, 7, 56
IMAGES = [
    # G = 8 > Q: two ground-truth objects (3 and 6) stay unmatched -> the reference's query 1;
    # relations [0,1,*] twice: a duplicated (subject query, object query) pair
    dict(gl=[3, 17, 90, 120, 3, 5, 60, 7],
         rels=[[0, 1, 5], [2, 3, 17], [3, 6, 56], [0, 1, 9], [6, 3, 1]],
         rows=[0, 1, 2, 3, 4, 5], cols=[7, 0, 5, 1, 2, 4],
         rows2=[0, 2, 3, 5, 6], cols2=[4, 0, 3, 1, 2]),
    # T = 1
    dict(gl=[5, 60, 7], rels=[[2, 0, 30]], rows=[1, 3, 4], cols=[2, 0, 1], rows2=[4], cols2=[0]),
    # every relation shares one class pair
    dict(gl=[11, 12, 11], rels=[[0, 1, 3], [0, 1, 7], [2, 1, 9], [0, 1, 3]],
         rows=[0, 2, 5], cols=[1, 2, 0], rows2=[1, 2, 4, 6], cols2=[3, 1, 0, 2]),
]


def run_targets(images, lsa_status=None, cum0=None):
    from pairnet_amd import hip
    B = len(images)
    lsa_tab, tgt_tab, gt, rows, cols = [], [], [], [], []
    for im in images:
        G, T = len(im["gl"]), len(im["rels"])
        lsa_tab.append([0, Q_, G, len(rows)])
        rows += im["rows"]
        cols += im["cols"]
        lsa_tab.append([0, R_, T, len(rows)])
        rows += im["rows2"]
        cols += im["cols2"]
        tgt_tab.append([len(gt), len(gt) + G, G, T])
        gt += list(im["gl"]) + [x for r in im["rels"] for x in r]
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=DEV)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    cum0 = np.zeros(C_ + 1, np.float32) if cum0 is None else cum0
    cum = torch.from_numpy(cum0.copy()).to(DEV)
    imp = torch.full((B, Q_, Q_), 9.0, device=DEV)
    labels = torch.full((3, B * R_), 9, dtype=torch.int64, device=DEV)
    bstatus = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        hip.loss_targets(i64(lsa_tab), i32(rows), i32(cols),
                         i32([0] * (2 * B) if lsa_status is None else lsa_status), i64(tgt_tab),
                         i64(gt), Q_, R_, imp, labels, cum, bstatus)
    return imp.cpu().numpy(), labels.cpu().numpy(), cum.cpu().numpy(), int(bstatus.cpu()[0])


def test_loss_targets_against_the_numpy_lines():
    rng = np.random.default_rng(40)
    cum0 = rng.integers(0, 50, C_ + 1).astype(np.float32)
    imp, labels, cum, st = run_targets(IMAGES, cum0=cum0)
    assert st == 0
    want_cum = cum0.copy()
    for b, im in enumerate(IMAGES):
        a = lambda k: np.asarray(im[k], dtype=np.int64)
        r, s, o, w_imp = numpy_targets(Q_, R_, a("gl"), a("rels"), a("rows"), a("cols"), a("rows2"),
                                       a("cols2"))
        assert np.array_equal(imp[b], w_imp), b
        for got, want in zip(labels[:, b * R_:(b + 1) * R_], (r, s, o)):
            assert np.array_equal(got, want), b
        np.add.at(want_cum, r[r >= 0], 1.0)
    assert np.array_equal(cum, want_cum)
    # the cases the images were built for
    assert imp[0][1, 1] == 1.0                 # two unmatched objects: (query 1, query 1)
    assert imp[0].sum() == 3.0                 # five relations on three distinct query pairs
    assert (labels[0, R_:2 * R_] >= 0).sum() == 1


def test_loss_targets_status():
    cum0 = np.arange(C_ + 1, dtype=np.float32)
    # an assignment that was refused: the fills only, the counts untouched, the statuses ORed
    imp, labels, cum, st = run_targets(IMAGES, lsa_status=[0, 0, 1, 0, 0, 2], cum0=cum0)
    assert st == 3 and (imp == 0).all() and (labels == -1).all() and np.array_equal(cum, cum0)
    # a ground-truth relation that names object 5 of 3
    bad = [dict(IMAGES[1], rels=[[5, 0, 30]])]
    imp, labels, cum, st = run_targets(bad, cum0=cum0)
    assert st == 4 and (imp == 0).all() and (labels == -1).all() and np.array_equal(cum, cum0)
