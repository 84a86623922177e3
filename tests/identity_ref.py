"""numpy restatement of the track-level identity measures (the definition in
include/tao_amodal_hip.h, section "track-level identity").  TEST INFRASTRUCTURE
ONLY.

The per-frame overlaps come from orclib.bb_iou, the C oracle the suite pins to
the reference's compiled bbIou (or from orclib.ref_bb_iou, that very function);
everything else is an integer.  The optimum of an assignment is unique, the
assignment is not: tests compare the counts with ``==`` and check an assignment
for validity and optimality (check_assignment), never for equality."""
import itertools
from types import SimpleNamespace

import numpy as np

import orclib
from track_error_types_ref import make_track_flat

GT_IGNORE = 1
DT_IGNORE_UNMATCHED = 1
CAT_COLUMNS = ("gt_tracks", "gt_frames", "dt_tracks", "dt_frames", "idtp", "pairs")
INF = np.int64(1) << 61


def share(f, frame_thr, bb_iou=None):
    """int32[n_iou]: per pair of a cell, the frames of the ground truth on which
    the detection track has a box with an overlap >= frame_thr."""
    assert 0 < frame_thr <= 1
    bb_iou = bb_iou or orclib.bb_iou
    d_off, g_off = np.asarray(f.cell_dt_off, np.int64), np.asarray(f.cell_gt_off, np.int64)
    ioff = np.asarray(f.cell_iou_off, np.int64)
    dfoff, gfoff = np.asarray(f.dt_frame_off, np.int64), np.asarray(f.gt_frame_off, np.int64)
    dfpos, gfpos = np.asarray(f.dt_frame_pos, np.int64), np.asarray(f.gt_frame_pos, np.int64)
    dfbox = np.asarray(f.dt_frame_box, dtype=np.float64).reshape(-1, 4)
    gfbox = np.asarray(f.gt_frame_box, dtype=np.float64).reshape(-1, 4)
    out = np.zeros(int(ioff[-1]), np.int32)
    for c in range(f.n_cells):
        d0, d1, g0, g1 = d_off[c], d_off[c + 1], g_off[c], g_off[c + 1]
        D, G = d1 - d0, g1 - g0
        if not D or not G:
            continue
        # the cell's detection frames by position
        fr = np.arange(dfoff[d0], dfoff[d1])
        owner = np.repeat(np.arange(D), np.diff(dfoff[d0:d1 + 1]))
        by_pos = np.argsort(dfpos[fr], kind="stable")
        c_pos, c_fr, c_own = dfpos[fr][by_pos], fr[by_pos], owner[by_pos]
        S = np.zeros((D, G), np.int32)
        for g in range(g0, g1):
            s, e = gfoff[g], gfoff[g + 1]
            lo = np.searchsorted(c_pos, gfpos[s:e], "left")
            hi = np.searchsorted(c_pos, gfpos[s:e], "right")
            for k in range(s, e):
                a, b = lo[k - s], hi[k - s]
                if a == b:
                    continue
                with np.errstate(all="ignore"):
                    v = bb_iou(dfbox[c_fr[a:b]], gfbox[k:k + 1])[:, 0]
                    ok = v >= frame_thr                 # (a NaN compares false: no overlap)
                # (a track has one frame at a position: no row twice)
                S[c_own[a:b][ok], g - g0] += 1
        out[ioff[c]:ioff[c] + D * G] = S.ravel()
    return out


def hungarian(w):
    """A maximum-weight assignment of the smaller side of w (int [n, m], entries
    >= 0) into the larger: (the optimum, row_to_col int64[n], -1 where the row
    has no column).  Shortest augmenting paths on cost = -w with potentials, the
    column loops as numpy expressions."""
    w = np.asarray(w, dtype=np.int64)
    n, m = w.shape
    if n == 0 or m == 0:
        return 0, -np.ones(n, np.int64)
    if n > m:
        total, col_to_row = hungarian(w.T)
        out = -np.ones(n, np.int64)
        out[col_to_row] = np.arange(m)
        return total, out
    cost = -w
    u, v = np.zeros(n + 1, np.int64), np.zeros(m + 1, np.int64)
    p, way = np.zeros(m + 1, np.int64), np.zeros(m + 1, np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(m + 1, INF)
        used = np.zeros(m + 1, bool)
        for _ in range(m + 1):
            used[j0] = True
            i0 = p[j0]
            free = ~used
            free[0] = False
            cur = cost[i0 - 1] - u[i0] - v[1:]
            better = free[1:] & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            j1 = 1 + int(np.argmin(np.where(free[1:], minv[1:], INF)))
            delta = minv[j1]
            assert free[j1] and delta < INF
            u[p[used]] += delta
            v[used] -= delta
            minv[free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        else:
            raise AssertionError("no augmenting path")
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    out = -np.ones(n, np.int64)
    cols = np.flatnonzero(p[1:])
    out[p[1:][cols] - 1] = cols
    return int(w[np.arange(n), out].sum()), out


def brute_force(w):
    """The optimum over all injections of the smaller side into the larger."""
    w = np.asarray(w, dtype=np.int64)
    if w.shape[0] > w.shape[1]:
        w = w.T
    n, m = w.shape
    if n == 0:
        return 0
    return max(int(w[np.arange(n), list(q)].sum()) for q in itertools.permutations(range(m), n))


def brute_force_pairs(w):
    """(the optimum, the most pairs with a positive weight among the assignments
    that reach it) over all injections of the smaller side into the larger."""
    w = np.asarray(w, dtype=np.int64)
    if w.shape[0] > w.shape[1]:
        w = w.T
    n, m = w.shape
    if n == 0:
        return 0, 0
    return max((int(w[np.arange(n), list(q)].sum()), int((w[np.arange(n), list(q)] > 0).sum()))
               for q in itertools.permutations(range(m), n))


def identity_from_share(t, sh):
    """t: cell_dt_off, cell_gt_off, cell_iou_off, gt_cat, gt_flags, dt_cat,
    dt_flags, dt_frame_off, gt_frame_off, cat_ids (a Flat has them).  Returns
    dict(cat_counts int64[K, 6], gt_ident int32[n_gt, 2], dt_ident int32[n_dt,
    2] -- ONE optimal assignment --, cell_idtp int64[n_cells], kept, eligible)."""
    d_off, g_off = np.asarray(t.cell_dt_off, np.int64), np.asarray(t.cell_gt_off, np.int64)
    ioff = np.asarray(t.cell_iou_off, np.int64)
    n_dt, n_gt, K = int(d_off[-1]), int(g_off[-1]), len(t.cat_ids)
    gt_cat, dt_cat = np.asarray(t.gt_cat, np.int64), np.asarray(t.dt_cat, np.int64)
    F = np.diff(np.asarray(t.dt_frame_off, np.int64))
    L = np.diff(np.asarray(t.gt_frame_off, np.int64))
    elig = (np.asarray(t.gt_flags)[:n_gt] & GT_IGNORE) == 0
    flagged = (np.asarray(t.dt_flags)[:n_dt] & DT_IGNORE_UNMATCHED) != 0
    kept = np.zeros(n_dt, bool)
    cat_counts = np.zeros((K, 6), np.int64)
    gt_ident = np.tile(np.array([-1, 0], np.int32), (n_gt, 1))
    dt_ident = np.tile(np.array([-1, 0], np.int32), (n_dt, 1))
    cell_idtp = np.zeros(len(d_off) - 1, np.int64)
    for c in range(len(d_off) - 1):
        d0, d1, g0, g1 = d_off[c], d_off[c + 1], g_off[c], g_off[c + 1]
        D, G = d1 - d0, g1 - g0
        S = np.asarray(sh[ioff[c]:ioff[c] + D * G], np.int64).reshape(D, G)
        e = elig[g0:g1]
        me = S[:, e].max(1) if e.any() else np.zeros(D, np.int64)
        mi = S[:, ~e].max(1) if (~e).any() else np.zeros(D, np.int64)
        k = ~(mi > me) & ~(flagged[d0:d1] & (me == 0))
        kept[d0:d1] = k
        rows, cols = np.flatnonzero(k), np.flatnonzero(e)
        # the sum of shares decides, then the number of pairs with a positive share
        W = S[np.ix_(rows, cols)]
        _, asg = hungarian(W * (min(W.shape) + 1) + (W > 0))
        cell_idtp[c] = int(W[np.flatnonzero(asg >= 0), asg[asg >= 0]].sum())
        for r, j in enumerate(asg):
            if j >= 0 and S[rows[r], cols[j]] > 0:
                d, g = d0 + rows[r], g0 + cols[j]
                gt_ident[g] = [d, S[rows[r], cols[j]]]
                dt_ident[d, 0] = g
                if 0 <= gt_cat[g] < K:
                    cat_counts[gt_cat[g], 4:] += [S[rows[r], cols[j]], 1]
    dt_ident[:, 1] = kept
    for g in np.flatnonzero(elig & (gt_cat[:n_gt] >= 0) & (gt_cat[:n_gt] < K)):
        cat_counts[gt_cat[g], :2] += [1, L[g]]
    for d in np.flatnonzero(kept & (dt_cat[:n_dt] >= 0) & (dt_cat[:n_dt] < K)):
        cat_counts[dt_cat[d], 2:4] += [1, F[d]]
    return dict(cat_counts=cat_counts, gt_ident=gt_ident, dt_ident=dt_ident,
                cell_idtp=cell_idtp, kept=kept, eligible=elig)


def identity(f, frame_thr, bb_iou=None):
    """identity_from_share on share(f, frame_thr), with "share" added."""
    sh = share(f, frame_thr, bb_iou)
    out = identity_from_share(f, sh)
    out["share"] = sh
    return out


def ratios(cat_counts):
    """(idf1, idp, idr) float64[K] of cat_counts[K, 6]; NaN where the denominator is 0."""
    c = np.asarray(cat_counts, dtype=np.float64)
    with np.errstate(all="ignore"):
        return (2 * c[..., 4] / (c[..., 1] + c[..., 3]), c[..., 4] / c[..., 3],
                c[..., 4] / c[..., 1])


def check_assignment(t, sh, want, gt_ident, dt_ident):
    """gt_ident / dt_ident are a valid one-to-one assignment inside the cells,
    over kept and eligible rows only, of pairs with a positive share, and every
    cell's shares add up to the optimum of `want` (identity_from_share)."""
    d_off, g_off = np.asarray(t.cell_dt_off, np.int64), np.asarray(t.cell_gt_off, np.int64)
    ioff = np.asarray(t.cell_iou_off, np.int64)
    n_dt, n_gt = int(d_off[-1]), int(g_off[-1])
    assert gt_ident.shape == (n_gt, 2) and dt_ident.shape == (n_dt, 2)
    assert gt_ident.dtype == np.int32 and dt_ident.dtype == np.int32
    assert np.array_equal(dt_ident[:, 1], want["kept"].astype(np.int32))
    for c in range(len(d_off) - 1):
        d0, d1, g0, g1 = d_off[c], d_off[c + 1], g_off[c], g_off[c + 1]
        G = g1 - g0
        gi, di = gt_ident[g0:g1].astype(np.int64), dt_ident[d0:d1].astype(np.int64)
        on = gi[:, 0] >= 0
        assert np.array_equal(gi[~on], np.tile([-1, 0], ((~on).sum(), 1))), c
        d = gi[on, 0]
        assert ((d >= d0) & (d < d1)).all(), c
        assert len(set(d.tolist())) == len(d), c                      # each d at most once
        assert want["eligible"][g0:g1][on].all() and want["kept"][d].all(), c
        g_loc = np.flatnonzero(on)
        s = np.asarray(sh, np.int64)[ioff[c] + (d - d0) * G + g_loc]
        assert (s > 0).all() and np.array_equal(s, gi[on, 1]), c
        # the detection side says the same
        back = -np.ones(d1 - d0, np.int64)
        back[d - d0] = g0 + g_loc
        assert np.array_equal(di[:, 0], back), c
        assert int(s.sum()) == int(want["cell_idtp"][c]), (c, int(s.sum()), want["cell_idtp"][c])


def table(cells, cat, gt_flags, dt_flags, n_cat, rng=None):
    """A table without frames' boxes for the assignment alone: cells = [(D, G)],
    cat[c] the category of cell c; frame counts 1 .. 9 from rng (1 without)."""
    D = np.array([c[0] for c in cells], np.int64)
    G = np.array([c[1] for c in cells], np.int64)
    t = SimpleNamespace()
    t.n_cells = len(cells)
    t.cell_dt_off = np.r_[0, np.cumsum(D)].astype(np.int32)
    t.cell_gt_off = np.r_[0, np.cumsum(G)].astype(np.int32)
    t.cell_iou_off = np.r_[0, np.cumsum(D * G)].astype(np.int64)
    t.dt_cat = np.repeat(np.asarray(cat, np.int32), D)
    t.gt_cat = np.repeat(np.asarray(cat, np.int32), G)
    t.gt_flags = np.asarray(gt_flags, np.uint8)
    t.dt_flags = np.asarray(dt_flags, np.uint8)
    fd = rng.integers(1, 10, int(D.sum())) if rng is not None else np.ones(int(D.sum()), np.int64)
    fg = rng.integers(1, 10, int(G.sum())) if rng is not None else np.ones(int(G.sum()), np.int64)
    t.dt_frame_off = np.r_[0, np.cumsum(fd)].astype(np.int32)
    t.gt_frame_off = np.r_[0, np.cumsum(fg)].astype(np.int32)
    t.cat_ids = np.arange(n_cat, dtype=np.int64)
    return t


# ---------------------------------------------------------------------------
# The hand-written table.  Ground truths 0 .. 2 and 4 have box [0, 0, 10, 10]
# everywhere, the ignored one (3) lies elsewhere.
# ---------------------------------------------------------------------------
BOX = [0, 0, 10, 10]
HALF = [0, 0, 10, 5]          # IoU with BOX: 50 / (100 + 50 - 50) = 0.5 exactly
LOW = [0, 0, 10, 4]           # 0.4
AWAY = [100, 100, 10, 10]     # 0 with BOX
HAND_THR = 0.5
HAND_THR_ABOVE = 0.5 + 2.0 ** -52     # HALF's overlap lies two units in the last place below

HAND_GTS = [
    # video 0: greedy by largest share takes (A, 0) = 5 and is left with (B, 1) = 0;
    # the optimum is (B, 0) + (A, 1) = 4 + 4
    (0, 0, {p: BOX for p in range(5)}, 0),                         # 0
    (0, 0, {p: BOX for p in range(10, 14)}, 0),                    # 1
    # video 1: an eligible and an ignored ground truth
    (1, 0, {p: BOX for p in range(4)}, 0),                         # 2
    (1, 0, {p: AWAY for p in range(6)}, GT_IGNORE),                # 3
    # video 3, category 1: a cell without detections
    (3, 1, {p: BOX for p in range(3)}, 0),                         # 4
]
HAND_DETS = [
    (0, 0, {**{p: BOX for p in range(5)}, **{p: BOX for p in range(10, 14)}}, 0.9, 0),   # 0  A
    (0, 0, {p: BOX for p in range(4)}, 0.8, 0),                                          # 1  B
    # C follows the ignored ground truth on 3 frames, the eligible one on 1: rule (a)
    (1, 0, {0: AWAY, 1: AWAY, 2: AWAY, 3: BOX}, 0.9, 0),                                 # 2  C
    # D is flagged and shares no frame (0.4 < frame_thr): rule (b)
    (1, 0, {0: LOW, 1: LOW}, 0.8, DT_IGNORE_UNMATCHED),                                  # 3  D
    # E is flagged and shares frames: it stays.  Frame 0 overlaps at exactly frame_thr
    (1, 0, {0: HALF, 1: BOX, 2: BOX}, 0.7, DT_IGNORE_UNMATCHED),                         # 4  E
    # video 2: a cell without ground truth.  H counts (false positives), I is flagged
    (2, 0, {0: BOX, 1: BOX}, 0.9, 0),                                                    # 5  H
    (2, 0, {0: BOX}, 0.8, DT_IGNORE_UNMATCHED),                                          # 6  I
    # J lies on ground truth 0, in another category: no candidate, counted in its own
    (0, 1, {p: BOX for p in range(5)}, 0.95, 0),                                         # 7  J
]
A, B, C_, D_, E, H, I_, J = range(8)
# share of the cell (video 0, category 0): [A, B] x [0, 1]; of (video 1, category 0):
# [C, D, E] x [2, 3]
HAND_SHARE_CELL0 = [[5, 4], [4, 0]]
HAND_SHARE_CELL1 = [[1, 3], [0, 0], [3, 0]]
HAND_SHARE_CELL1_ABOVE = [[1, 3], [0, 0], [2, 0]]
HAND_GREEDY_CELL0, HAND_IDTP_CELL0 = 5, 8
# per ground truth given: {the detection given or -1, share}
HAND_GT_IDENT = [[B, 4], [A, 4], [E, 3], [-1, 0], [-1, 0]]
HAND_GT_IDENT_ABOVE = [[B, 4], [A, 4], [E, 2], [-1, 0], [-1, 0]]
# per detection given: {the ground truth given or -1, kept}
HAND_DT_IDENT = [[1, 1], [0, 1], [-1, 0], [-1, 0], [2, 1], [-1, 1], [-1, 0], [-1, 1]]
# category 0: ground truths 0, 1, 2 (5 + 4 + 4 frames); A, B, E, H kept (9 + 4 + 3 + 2
# frames); idtp 8 + 3.  Category 1: ground truth 4 (3 frames), J (5 frames)
HAND_CAT_COUNTS = [[3, 13, 4, 18, 11, 3], [1, 3, 1, 5, 0, 0]]
HAND_CAT_COUNTS_ABOVE = [[3, 13, 4, 18, 10, 3], [1, 3, 1, 5, 0, 0]]
HAND_IDF1 = [2 * 11 / (13 + 18), 0.0]
HAND_IDP = [11 / 18, 0.0]
HAND_IDR = [11 / 13, 0.0]


def hand_flat():
    """(flat, dt_at, gt_at)."""
    return make_track_flat(4, 2, HAND_DETS, HAND_GTS)


def by_given(got, dt_at, gt_at):
    """(gt_ident, dt_ident) in the order the tracks were given, rows as the
    numbers of the tracks given."""
    d_inv = {int(r): i for i, r in enumerate(dt_at)}
    g_inv = {int(r): i for i, r in enumerate(gt_at)}
    gi = [[d_inv.get(int(a), -1), int(b)] for a, b in got["gt_ident"][gt_at]]
    di = [[g_inv.get(int(a), -1), int(b)] for a, b in got["dt_ident"][dt_at]]
    return gi, di
