"""numpy restatement of the track-level association (the definition in
include/tao_amodal_hip.h, section "track-level association").  TEST
INFRASTRUCTURE ONLY.

The per-frame overlaps come from orclib.bb_iou, the C oracle the suite pins to
the reference's compiled bbIou (or from orclib.ref_bb_iou, that very function);
everything else is an integer: every comparison against the device is ``==``."""
import numpy as np

import orclib
from track_error_types_ref import make_track_flat

GT_IGNORE = 1
TRACK_COLUMNS = ("frames", "covered", "ids", "switches", "fragments", "primary",
                 "primary_frames")
CAT_COLUMNS = ("tracks", "frames", "covered", "ids", "switches", "fragments",
               "mostly_tracked", "mostly_lost")
# the image level's first five windows: all, highly-occluded, partially-occluded,
# highly-visible, highly-and-partially-occluded
VIS_RNG = [[0, 1.0], [0, 0.1], [0.1, 0.8], [0.8, 1.0], [0, 0.8]]


def association(f, vis, frame_thr, vis_rng=VIS_RNG, bb_iou=None):
    """f: a Flat of the track level (use_cats = 1); vis float64[n_gt_frames].
    Returns dict(follow int32[n_iou], gt_assoc int32[n_gt, 7] (primary: a table
    row), cat_counts int64[K, 8], vis_counts int64[n_vis, K, 3], best
    int32[n_gt_frames] (in-cell index), best_iou float64[n_gt_frames])."""
    assert 0 < frame_thr <= 1
    bb_iou = bb_iou or orclib.bb_iou
    d_off, g_off = np.asarray(f.cell_dt_off, np.int64), np.asarray(f.cell_gt_off, np.int64)
    ioff = np.asarray(f.cell_iou_off, np.int64)
    dfoff, gfoff = np.asarray(f.dt_frame_off, np.int64), np.asarray(f.gt_frame_off, np.int64)
    dfpos, gfpos = np.asarray(f.dt_frame_pos, np.int64), np.asarray(f.gt_frame_pos, np.int64)
    dfbox = np.asarray(f.dt_frame_box, dtype=np.float64).reshape(-1, 4)
    gfbox = np.asarray(f.gt_frame_box, dtype=np.float64).reshape(-1, 4)
    gt_cat, gt_flags = np.asarray(f.gt_cat), np.asarray(f.gt_flags)
    vis = np.asarray(vis, dtype=np.float64)
    vis_rng = np.asarray(vis_rng, dtype=np.float64).reshape(-1, 2)
    n_gt, K = int(g_off[-1]), len(f.cat_ids)
    assert len(vis) == len(gfpos)
    follow = np.zeros(int(ioff[-1]), np.int32)
    gt_assoc = np.zeros((n_gt, 7), np.int32)
    cat_counts = np.zeros((K, 8), np.int64)
    vis_counts = np.zeros((len(vis_rng), K, 3), np.int64)
    best = -np.ones(len(gfpos), np.int32)
    best_iou = np.zeros(len(gfpos))
    for c in range(f.n_cells):
        d0, d1, g0, g1 = d_off[c], d_off[c + 1], g_off[c], g_off[c + 1]
        D, G = d1 - d0, g1 - g0
        # the cell's detection frames by position, rows ascending within a position
        fr = np.arange(dfoff[d0], dfoff[d1])
        owner = np.repeat(np.arange(D), np.diff(dfoff[d0:d1 + 1]))
        by_pos = np.argsort(dfpos[fr], kind="stable")
        c_pos, c_fr, c_own = dfpos[fr][by_pos], fr[by_pos], owner[by_pos]
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
                if ok.any():
                    at = int(np.argmax(np.where(ok, v, -np.inf)))    # the first = the lowest row
                    best[k], best_iou[k] = c_own[a + at], v[at]
            bk = best[s:e]
            cov = bk[bk >= 0]
            count = np.bincount(cov, minlength=D) if D else np.zeros(0, np.int64)
            follow[ioff[c] + np.arange(D) * G + (g - g0)] = count
            covered = len(cov)
            frag = int(np.sum((bk >= 0) & np.r_[True, bk[:-1] < 0]))
            prim = int(np.argmax(count)) if covered else -1          # the first = the lowest row
            gt_assoc[g] = [e - s, covered, int((count > 0).sum()), int((cov[1:] != cov[:-1]).sum()),
                           frag, d0 + prim if covered else -1, count[prim] if covered else 0]
            if gt_flags[g] & GT_IGNORE:
                continue
            L = int(e - s)
            cat_counts[gt_cat[g]] += [1, L, covered] + gt_assoc[g, 2:5].tolist() \
                + [5 * covered >= 4 * L, 5 * covered < L]
            for w, (vlo, vhi) in enumerate(vis_rng):
                inside = (vlo <= vis[s:e]) & (vis[s:e] <= vhi)       # (a NaN is in no window)
                vis_counts[w, gt_cat[g]] += [int(inside.sum()), int((inside & (bk >= 0)).sum()),
                                             int((inside & (bk >= 0) & (bk == prim)).sum())]
    return dict(follow=follow, gt_assoc=gt_assoc, cat_counts=cat_counts, vis_counts=vis_counts,
                best=best, best_iou=best_iou)


def frame_vis(f, gt_at, per_gt):
    """float64[n_gt_frames] from {position: visibility} of the i-th ground truth
    given (tracks in table order, frames by ascending position)."""
    out = np.zeros(int(f.gt_frame_off[-1]))
    for i, vis in enumerate(per_gt):
        s = int(f.gt_frame_off[gt_at[i]])
        for j, p in enumerate(sorted(vis)):
            assert f.gt_frame_pos[s + j] == p
            out[s + j] = vis[p]
    return out


# ---------------------------------------------------------------------------
# The hand-written table.  The ground truth's box is [0, 0, 10, 10] everywhere.
# ---------------------------------------------------------------------------
BOX = [0, 0, 10, 10]
HALF = [0, 0, 10, 5]          # IoU with BOX: 50 / (100 + 50 - 50) = 0.5 exactly
LOW = [0, 0, 10, 4]           # 0.4
AWAY = [100, 100, 10, 10]     # 0
NAN = float("nan")
HAND_THR = 0.5
HAND_THR_ABOVE = 0.5 + 2.0 ** -52

HAND_GTS = [
    # 0: six frames followed A, A, -, B, A, A
    (0, 0, {p: BOX for p in range(6)}, 0),
    # 1: four of six frames covered, by two detection tracks with identical boxes
    (1, 0, {p: BOX for p in range(6)}, 0),
    # 2: frame 0 overlaps at exactly frame_thr; a track of category 1 lies on top of it
    (2, 0, {0: BOX, 1: BOX}, 0),
    # 3: a cell without detections
    (3, 0, {0: BOX, 1: BOX, 2: BOX}, 0),
    # 4: "ignore", in the cell of 0: in gt_assoc, in no count table
    (0, 0, {0: BOX, 1: BOX}, GT_IGNORE),
]
HAND_VIS = [
    # 0.1 and 0.8 lie in both neighbouring windows, the NaN in none
    {0: 0.1, 1: 0.8, 2: 0.05, 3: 0.5, 4: NAN, 5: 1.0},
    {p: 1.0 for p in range(6)},
    {0: 0.9, 1: 0.9},
    {0: 0.0, 1: 0.0, 2: 0.0},
    {0: 0.5, 1: 0.5},
]
HAND_DETS = [
    (0, 0, {0: BOX, 1: BOX, 2: AWAY, 4: BOX, 5: BOX}, 0.9, 0),     # 0  A
    (0, 0, {2: LOW, 3: BOX}, 0.8, 0),                              # 1  B
    (1, 0, {p: BOX for p in range(4)}, 0.7, 0),                    # 2  C: the lower row
    (1, 0, {p: BOX for p in range(4)}, 0.6, 0),                    # 3  D: C's copy
    (2, 0, {0: HALF, 1: BOX}, 0.9, 0),                             # 4  E
    (2, 1, {0: BOX, 1: BOX}, 0.95, 0),                             # 5  F: another category
]
A, B, C_, D_, E, F = range(6)
# gt_assoc per ground truth given, `primary` as the number of the detection given
HAND_ASSOC = [[6, 5, 2, 2, 2, A, 4], [6, 4, 1, 0, 1, C_, 4], [2, 2, 1, 0, 1, E, 2],
              [3, 0, 0, 0, 0, -1, 0], [2, 2, 1, 0, 1, A, 2]]
# at frame_thr + 2 ** -52 frame 0 of ground truth 2 is not covered
HAND_ASSOC_ABOVE_GT2 = [2, 1, 1, 0, 1, E, 1]
# best per frame of ground truths 0 and 4 (cell (0, 0): A is in-cell 0, B is 1)
HAND_BEST_GT0 = [0, 0, -1, 1, 0, 0]
HAND_BEST_IOU_GT0 = [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]
# follow of cell (video 0, category 0): [A, B] x [ground truth 0, ground truth 4]
HAND_FOLLOW_CELL0 = [[4, 2], [1, 0]]
# category 0: ground truths 0 .. 3; 0 (5 / 6) and 2 are mostly tracked, 1 (4 / 6) is
# not, 3 is mostly lost; category 1 has no ground truth
HAND_CAT_COUNTS = [[4, 17, 11, 4, 2, 4, 2, 1], [0] * 8]
HAND_CAT_COUNTS_ABOVE = [[4, 17, 10, 4, 2, 4, 1, 1], [0] * 8]
# category 0 per window of VIS_RNG: frames, covered, followed by the primary
HAND_VIS_COUNTS = [[16, 10, 9], [5, 1, 1], [3, 3, 2], [10, 8, 8], [7, 3, 2]]


def hand_flat():
    """(flat, dt_at, gt_at, vis)."""
    f, dt_at, gt_at = make_track_flat(4, 2, HAND_DETS, HAND_GTS)
    return f, dt_at, gt_at, frame_vis(f, gt_at, HAND_VIS)


# ---------------------------------------------------------------------------
# The empty sides: tables of two categories and at most three cells for the
# association and the identity's share pass, which build one frame index.
# ---------------------------------------------------------------------------
def side_table(cells, dts, gts, first=(0, 0), loose=0):
    """A table written row by row, so that it can hold what no flatten makes.
    cells: (detection tracks, ground-truth tracks) per cell, dts: {position:
    box} per detection row, gts: (category, flags, {position: box}) per ground-
    truth row; first = (detection rows, ground-truth rows) before the first
    cell's -- rows no cell lists; loose: ground-truth frames behind the last
    track's -- frames no track lists.  Returns (table, vis)."""
    from types import SimpleNamespace

    def frames(tracks, extra=0):
        pos = [p for fr in tracks for p in sorted(fr)] + list(range(extra))
        box = [fr[p] for fr in tracks for p in sorted(fr)] + [BOX] * extra
        return (np.cumsum([0] + [len(fr) for fr in tracks]).astype(np.int32),
                np.array(pos, np.int32), np.array(box, np.float64).reshape(-1, 4))
    D = np.array([c[0] for c in cells], np.int64)
    G = np.array([c[1] for c in cells], np.int64)
    f = SimpleNamespace(n_cells=len(cells), cat_ids=np.arange(2, dtype=np.int64))
    f.cell_dt_off = (first[0] + np.r_[0, np.cumsum(D)]).astype(np.int32)
    f.cell_gt_off = (first[1] + np.r_[0, np.cumsum(G)]).astype(np.int32)
    f.cell_iou_off = np.r_[0, np.cumsum(D * G)].astype(np.int64)
    assert f.cell_dt_off[-1] == len(dts) and f.cell_gt_off[-1] == len(gts)
    f.gt_cat = np.array([g[0] for g in gts], np.int32)
    f.gt_flags = np.array([g[1] for g in gts], np.uint8)
    f.dt_frame_off, f.dt_frame_pos, f.dt_frame_box = frames(dts)
    f.gt_frame_off, f.gt_frame_pos, f.gt_frame_box = frames([g[2] for g in gts], loose)
    # (a visibility per frame that lies in some windows of VIS_RNG and not in others)
    return f, np.resize([0.05, 0.5, 0.9, 1.0], len(f.gt_frame_pos))


def _run(positions, box=BOX):
    return {p: box for p in positions}


def empty_sides():
    """{case: (table, vis)}.  A ground-truth row no cell lists is marked "ignore":
    the restatement walks the cells and never sees it, so it may count nowhere."""
    one, long_ = _run(range(1)), _run(range(65))
    some = [_run(range(3)), _run(range(2, 70)), _run((0, 64))]
    out = {
        # (a) no detection tracks at all, ground-truth tracks of 1 and 65 frames
        "no_detection_tracks": side_table([(0, 1), (0, 1)], [], [(0, 0, one), (1, 0, long_)]),
        # (b) no ground-truth tracks
        "no_ground_truth": side_table([(2, 0), (1, 0)], some, []),
        # (c) no cells, rows on both sides
        "no_cells": side_table([], some, [(0, GT_IGNORE, one), (1, GT_IGNORE, long_)],
                               first=(3, 2)),
        # (d) detection tracks that all have no frames
        "no_detection_frames": side_table([(2, 1), (1, 1)], [{}, {}, {}],
                                          [(0, 0, one), (1, 0, long_)]),
    }
    # (e) ground-truth row 0 is in no cell, the last two ground-truth frames in no
    # track; of the first cell's detection tracks the middle one has no frames and
    # the last a hole at position 10 between its ends 0 and 20, where the ground
    # truth has a frame: the probe bisects.  HALF overlaps at exactly 0.5.
    holed = {**_run(range(10), HALF), **_run(range(11, 21), HALF)}
    out["mixed"] = side_table(
        [(3, 1), (1, 1)], [_run(range(10)), {}, holed, _run((6, 7, 8))],
        [(0, GT_IGNORE, _run(range(2))), (0, 0, long_), (1, 0, _run((5, 6, 7)))],
        first=(0, 1), loose=2)
    return out


def association_of_table(f, vis, frame_thr):
    """association() for a table of side_table(): a ground-truth row no cell lists
    is not the restatement's to visit; its row of gt_assoc is the header's "no
    candidates" -- its frames, nothing covered, no primary."""
    want = association(f, vis, frame_thr)
    g_off = np.asarray(f.cell_gt_off, np.int64)
    listed = np.zeros(int(g_off[-1]), bool)
    for c in range(f.n_cells):
        listed[g_off[c]:g_off[c + 1]] = True
    for g in np.flatnonzero(~listed):
        assert f.gt_flags[g] & GT_IGNORE
        want["gt_assoc"][g] = [f.gt_frame_off[g + 1] - f.gt_frame_off[g], 0, 0, 0, 0, -1, 0]
    return want
