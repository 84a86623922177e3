"""The track-level identity measures without a GPU: the numpy restatement
(tests/identity_ref.py) on the hand-written table with literal expectations,
its Hungarian against brute force (and scipy where installed), and the C ABI's
new symbols and refusals (argument and workspace checks come before the first
device call)."""
import os
import re

import numpy as np
import pytest

import identity_ref as ref
from tao_amodal_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cell(f, got, g_row):
    k = int(f.gt_cell[g_row])
    D = f.cell_dt_off[k + 1] - f.cell_dt_off[k]
    G = f.cell_gt_off[k + 1] - f.cell_gt_off[k]
    return k, got["share"][f.cell_iou_off[k]:f.cell_iou_off[k + 1]].reshape(D, G)


def test_restatement_reproduces_the_literals():
    f, dt_at, gt_at = ref.hand_flat()
    got = ref.identity(f, ref.HAND_THR)
    k0, s0 = _cell(f, got, gt_at[0])
    k1, s1 = _cell(f, got, gt_at[2])
    assert s0.tolist() == ref.HAND_SHARE_CELL0 and s1.tolist() == ref.HAND_SHARE_CELL1
    # greedy by largest share loses: it takes 5 and is left with 0
    assert max(map(max, ref.HAND_SHARE_CELL0)) + ref.HAND_SHARE_CELL0[1][1] == ref.HAND_GREEDY_CELL0
    assert got["cell_idtp"][k0] == ref.HAND_IDTP_CELL0 > ref.HAND_GREEDY_CELL0
    assert got["cell_idtp"][k1] == 3
    gi, di = ref.by_given(got, dt_at, gt_at)
    assert gi == ref.HAND_GT_IDENT and di == ref.HAND_DT_IDENT
    assert got["cat_counts"].tolist() == ref.HAND_CAT_COUNTS
    idf1, idp, idr = ref.ratios(got["cat_counts"])
    assert idf1.tolist() == ref.HAND_IDF1 and idp.tolist() == ref.HAND_IDP
    assert idr.tolist() == ref.HAND_IDR
    ref.check_assignment(f, got["share"], got, got["gt_ident"], got["dt_ident"])
    # the rules, one by one: (a) C follows the ignored ground truth more than the eligible one
    assert f.gt_flags[gt_at[3]] & ref.GT_IGNORE and not got["kept"][dt_at[ref.C_]]
    assert ref.HAND_SHARE_CELL1[0][1] > ref.HAND_SHARE_CELL1[0][0] > 0
    # (b) D and I are flagged and share nothing; E is flagged and stays; H is a false positive
    for d in (ref.D_, ref.E, ref.I_):
        assert f.dt_flags[dt_at[d]] & ref.DT_IGNORE_UNMATCHED
    assert not got["kept"][dt_at[ref.D_]] and not got["kept"][dt_at[ref.I_]]
    assert got["kept"][dt_at[ref.E]] and got["kept"][dt_at[ref.H]]
    # the cell without ground truth counts its kept track, the one without detections its frames
    cells = list(zip(np.diff(f.cell_dt_off).tolist(), np.diff(f.cell_gt_off).tolist()))
    assert (2, 0) in cells and (0, 1) in cells
    # J (category 1) lies on ground truth 0 (category 0) and is no candidate
    assert f.dt_cat[dt_at[ref.J]] == 1 and got["dt_ident"][dt_at[ref.J]].tolist() == [-1, 1]


def test_restatement_at_the_threshold_and_just_above():
    f, dt_at, gt_at = ref.hand_flat()
    at, above = ref.identity(f, ref.HAND_THR), ref.identity(f, ref.HAND_THR_ABOVE)
    assert _cell(f, above, gt_at[2])[1].tolist() == ref.HAND_SHARE_CELL1_ABOVE
    assert _cell(f, above, gt_at[0])[1].tolist() == ref.HAND_SHARE_CELL0
    assert ref.by_given(above, dt_at, gt_at)[0] == ref.HAND_GT_IDENT_ABOVE
    assert ref.by_given(above, dt_at, gt_at)[1] == ref.HAND_DT_IDENT
    assert above["cat_counts"].tolist() == ref.HAND_CAT_COUNTS_ABOVE
    assert (at["share"] >= above["share"]).all()


def test_share_is_at_least_the_associations_follow():
    import association_ref
    f, _, _ = ref.hand_flat()
    vis = np.zeros(len(f.gt_frame_pos))
    for thr in (ref.HAND_THR, ref.HAND_THR_ABOVE):
        follow = association_ref.association(f, vis, thr, vis_rng=[])["follow"]
        got = ref.share(f, thr)
        assert (got >= follow).all() and (got > follow).any()


def test_hungarian_against_brute_force():
    """300 random matrices of up to 5 x 6 with entries 0 .. 3: ties everywhere."""
    rng = np.random.default_rng(5)
    shapes = set()
    for _ in range(300):
        n, m = int(rng.integers(0, 6)), int(rng.integers(0, 7))
        w = rng.integers(0, 4, (n, m))
        total, asg = ref.hungarian(w)
        assert total == ref.brute_force(w), w
        on = asg >= 0
        assert on.sum() == min(n, m) and len(set(asg[on].tolist())) == on.sum()
        assert total == int(w[np.flatnonzero(on), asg[on]].sum())
        shapes.add((n, m))
    assert (5, 6) in shapes and any(n > m > 0 for n, m in shapes)
    assert ref.hungarian(ref.HAND_SHARE_CELL0)[0] == ref.HAND_IDTP_CELL0


def test_pairs_are_the_most_an_optimal_assignment_has():
    """[[2, 1], [1, 0]]: 2 + 0 and 1 + 1 both reach 2; the pairs with a positive
    share are counted on the assignment that has most of them, so that the count
    is unique.  Against brute force on single cells with ties everywhere."""
    rng = np.random.default_rng(8)
    mats = [np.array([[2, 1], [1, 0]])] + [
        rng.integers(0, 3, (int(rng.integers(1, 6)), int(rng.integers(1, 7)))) for _ in range(150)]
    for w in mats:
        D, G = w.shape
        t = ref.table([(D, G)], [0], np.zeros(G, np.uint8), np.zeros(D, np.uint8), 1)
        got = ref.identity_from_share(t, w.ravel())
        assert (int(got["cell_idtp"][0]), int(got["cat_counts"][0, 5])) == ref.brute_force_pairs(w)
        assert got["cat_counts"][0, 4] == got["cell_idtp"][0]
        ref.check_assignment(t, w.ravel(), got, got["gt_ident"], got["dt_ident"])
    assert ref.brute_force_pairs(mats[0]) == (2, 2)


def test_hungarian_against_scipy():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(6)
    for n, m, top in [(1, 1, 3), (7, 5, 3), (64, 65, 9), (65, 257, 9), (257, 65, 2 ** 30),
                      (63, 63, 1), (40, 200, 2)]:
        w = rng.integers(0, top + 1, (n, m))
        w[rng.random((n, m)) < 0.5] = 0
        r, c = opt.linear_sum_assignment(w, maximize=True)
        total, asg = ref.hungarian(w)
        assert total == int(w[r, c].sum()), (n, m)
        on = asg >= 0
        assert on.sum() == min(n, m) and len(set(asg[on].tolist())) == on.sum()


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    lib = _lib.load()
    for name in ("taoamd_track_identity_workspace", "taoamd_track_identity_share",
                 "taoamd_track_identity_assign"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert lib.taoamd_version() >= 110
    assert _lib.IDENT_CAT_COLUMNS == ref.CAT_COLUMNS and len(ref.CAT_COLUMNS) == 6


def test_abi_refusals_come_before_the_first_device_call():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    n_dt, n_gt, n_gf = 1000, 70, 3000
    need = int(lib.taoamd_track_identity_workspace(n_dt, n_gt, n_gf))
    # the association's three tables and the search state of every row
    assert need > 16 * n_dt + 4 * n_gt + 4 * n_gf + 40 * (n_dt + n_gt)
    for bad in ((-1, n_gt, n_gf), (n_dt, -1, n_gf), (n_dt, n_gt, -1), (2 ** 31, n_gt, n_gf)):
        assert lib.taoamd_track_identity_workspace(*bad) == 0

    def share(frame_thr=0.5, sizes=(n_dt, n_gt, 50, 4000, 9000, n_gf), nbytes=need - 1,
              ptrs=None):
        return lib.taoamd_track_identity_share(*sizes, frame_thr, *(ptrs or [p] * 11), nbytes,
                                               None)

    def assign(n_cat=7, sizes=(n_dt, n_gt, 50, 4000, 9000, n_gf), nbytes=need - 1, ptrs=None):
        return lib.taoamd_track_identity_assign(*sizes, n_cat, *(ptrs or [p] * 15), nbytes, None)
    for bad in (0.0, -0.1, 1 + 2.0 ** -52, float("nan")):
        assert share(frame_thr=bad) == 2, bad
    assert assign(n_cat=0) == 2 and assign(n_cat=-1) == 2
    for i in range(6):
        sizes = [n_dt, n_gt, 50, 4000, 9000, n_gf]
        sizes[i] = -1
        assert share(sizes=sizes) == 2 and assign(sizes=sizes) == 2, i
    # a missing table: every pointer in turn
    for i in range(11):
        ptrs = [p] * 11
        ptrs[i] = None
        assert share(ptrs=ptrs) == 2, i
    for i in range(15):
        ptrs = [p] * 15
        ptrs[i] = None
        assert assign(ptrs=ptrs) == 2, i
    # good arguments, one byte short: the workspace check, still no device call
    assert share() == 4 and share(frame_thr=1.0) == 4 and share(frame_thr=2.0 ** -1074) == 4
    assert assign() == 4 and assign(n_cat=1) == 4
