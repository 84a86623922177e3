"""numpy restatement of track-level CLEAR (the definition in
include/tao_amodal_hip.h, section "track-level CLEAR"), its three stages in the
kernel's order of operations.  TEST INFRASTRUCTURE ONLY.

The frame groups, q, c(s) and the assignment routine are those of
tests/hota_ref.py and tests/identity_ref.py, imported and not edited: the
algorithm and the tie rule of the kernel, so the pairs are compared with ``==``.
walk() and reduce() read the candidate store alone, never a box, as the device
stages do.

clear_float() is a second, independent statement from the definition in plain
float64 (TrackEval's CLEAR: 1000 * continuity + IoU) with
scipy.optimize.linear_sum_assignment per step."""
import numpy as np

import identity_ref
from hota_ref import (AWAY, BOX, GT_IGNORE, HALF, ONE, _eligible, cs, frame_counts,
                      frame_groups, q)
from track_error_types_ref import make_track_flat

BONUS = 1000 * ONE
TRACK_COLUMNS = ("present", "matched", "idsw", "started")
CAT_COLUMNS = ("tp", "idsw", "frag", "mt", "pt", "ml", "motp_sum")
VIS_COLUMNS = ("frames", "matched", "idsw", "q_sum")
RATIOS = ("mota", "motp", "moda", "smota", "clr_re", "clr_pr", "clr_f1", "mtr", "ptr", "mlr")


# ---------------------------------------------------------------------------
# stage 1: the candidates
# ---------------------------------------------------------------------------
def candidates(t, frame_thr, dt_keep=None, bb_iou=None):
    """dict(cand_off int64[n_gt_frames + 1], cand_row int32, cand_q int32,
    cand_iou float64, step uint8[n_gt_frames])."""
    assert 0 < frame_thr <= 1
    n_gf = len(np.asarray(t.gt_frame_pos))
    rows = [[] for _ in range(n_gf)]
    step = np.zeros(n_gf, np.uint8)
    for _, _, _, gf, dl, _, S in frame_groups(t, dt_keep, bb_iou):
        if not len(dl):
            continue
        step[gf] = 1
        with np.errstate(all="ignore"):
            on = (S >= frame_thr) & (q(cs(S)) > 0)           # (a NaN compares false)
        for i, k in enumerate(gf):
            rows[k] = [(int(dl[j]), int(q(cs(S[j, i]))), float(S[j, i]))
                       for j in np.flatnonzero(on[:, i])]
    off = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64)
    flat = [c for r in rows for c in r]
    return dict(cand_off=off, cand_row=np.array([c[0] for c in flat], np.int32),
                cand_q=np.array([c[1] for c in flat], np.int32),
                cand_iou=np.array([c[2] for c in flat], np.float64), step=step)


# ---------------------------------------------------------------------------
# stage 2: the chain
# ---------------------------------------------------------------------------
def _list(c, k, D):
    """The valid candidates of frame k: [(row, q, place)], q read as the walk reads it."""
    out = []
    for x in range(int(c["cand_off"][k]), int(c["cand_off"][k + 1])):
        row, qv = int(c["cand_row"][x]), int(c["cand_q"][x])
        if 0 <= row < D and qv > 0:
            out.append((row, min(qv, ONE), x))
    return out


def walk(t, c):
    """dict(match int32[n_gt_frames], match_iou, sw uint8, gt_clear int32[n_gt, 4],
    steps): steps = [(cell, p, gf, cols, W int64[rows, cols] with the bonus, prevs,
    pairs, stepno)] for every step with a candidate -- gf the frames of the rows,
    cols the in-cell detection rows, pairs = [(i, j)], stepno the step's number
    in its cell from 1."""
    d_off, g_off = np.asarray(t.cell_dt_off, np.int64), np.asarray(t.cell_gt_off, np.int64)
    gfoff, gfpos = np.asarray(t.gt_frame_off, np.int64), np.asarray(t.gt_frame_pos, np.int64)
    elig = _eligible(t)
    n_gf, n_gt = len(gfpos), int(g_off[-1])
    has_iou = c.get("cand_iou") is not None
    match, iou = -np.ones(n_gf, np.int32), np.zeros(n_gf)
    sw, gt_clear = np.zeros(n_gf, np.uint8), np.zeros((n_gt, 4), np.int32)
    steps = []
    for cell in range(len(d_off) - 1):
        D = int(d_off[cell + 1] - d_off[cell])
        rows = [g for g in range(g_off[cell], g_off[cell + 1]) if elig[g]]
        last, lstep = {g: -1 for g in rows}, {g: -1 for g in rows}
        for g in rows:
            gt_clear[g, 0] = gfoff[g + 1] - gfoff[g]
        at = {}
        for g in rows:                                       # (ascending row at a position)
            for k in range(gfoff[g], gfoff[g + 1]):
                at.setdefault(int(gfpos[k]), []).append((g, k))
        stepno = 0
        for p in sorted(at):
            here = at[p]
            if not c["step"][here[0][1]]:
                continue                                     # no step: no state changes
            stepno += 1
            lists = [(g, k, _list(c, k, D)) for g, k in here
                     if c["cand_off"][k + 1] > c["cand_off"][k]]
            cols = sorted({r for _, _, ls in lists for r, _, _ in ls})
            if not lists or not cols:
                continue
            W = np.zeros((len(lists), len(cols)), np.int64)
            X = np.zeros(W.shape, np.int64)
            prevs = []
            for i, (g, k, ls) in enumerate(lists):
                prev = last[g] if lstep[g] == stepno - 1 else -1
                prevs.append(prev)
                for r, qv, x in reversed(ls):                # (the first of equal rows holds)
                    W[i, cols.index(r)] = qv + (BONUS if r == prev else 0)
                    X[i, cols.index(r)] = x
            # (hungarian takes the smaller side as rows, the first when equal)
            _, asg = identity_ref.hungarian(W)
            pairs = [(i, int(j)) for i, j in enumerate(asg) if j >= 0 and W[i, j] > 0]
            for i, j in pairs:
                g, k, _ = lists[i]
                d = cols[j]
                match[k] = d
                iou[k] = c["cand_iou"][X[i, j]] if has_iou else 0.0
                if last[g] >= 0 and last[g] != d:
                    sw[k] = 1
                    gt_clear[g, 2] += 1
                gt_clear[g, 3] += lstep[g] != stepno - 1
                last[g], lstep[g] = d, stepno
                gt_clear[g, 1] += 1
            steps.append((cell, p, [k for _, k, _ in lists], cols, W, prevs, pairs, stepno))
    return dict(match=match, match_iou=iou, sw=sw, gt_clear=gt_clear, steps=steps)


# ---------------------------------------------------------------------------
# stage 3: the tables
# ---------------------------------------------------------------------------
def reduce(t, c, match, sw, gt_clear, vis=None, vis_rng=None, n_cat=None):
    """(cat_counts int64[K, 7], vis_counts int64[n_vis, K, 4])."""
    n_cat = len(t.cat_ids) if n_cat is None else n_cat
    gfoff = np.asarray(t.gt_frame_off, np.int64)
    elig, gt_cat = _eligible(t), np.asarray(t.gt_cat, np.int64)
    vis_rng = np.asarray(vis_rng if vis_rng is not None else [], np.float64).reshape(-1, 2)
    cat_counts = np.zeros((n_cat, 7), np.int64)
    vis_counts = np.zeros((len(vis_rng), n_cat, 4), np.int64)
    gt_clear = np.asarray(gt_clear, np.int64)
    for g in np.flatnonzero(elig):
        k_ = int(gt_cat[g])
        if not 0 <= k_ < n_cat:
            continue
        present, matched, idsw, started = gt_clear[g]
        mt = 5 * matched > 4 * present
        pt = (not mt) and 5 * matched >= present
        qs = np.zeros(gfoff[g + 1] - gfoff[g], np.int64)
        for n, k in enumerate(range(gfoff[g], gfoff[g + 1])):
            if match[k] >= 0:
                for x in range(int(c["cand_off"][k]), int(c["cand_off"][k + 1])):
                    if c["cand_row"][x] == match[k]:
                        qv = int(c["cand_q"][x])
                        qs[n] = min(qv, ONE) if qv > 0 else 0
                        if qs[n]:
                            break
        cat_counts[k_] += [max(matched, 0), max(idsw, 0), max(started - 1, 0), mt, pt,
                           not mt and not pt, qs.sum()]
        m = np.asarray(match[gfoff[g]:gfoff[g + 1]]) >= 0
        s = np.asarray(sw[gfoff[g]:gfoff[g + 1]]) != 0
        for w, (lo, hi) in enumerate(vis_rng):
            v = np.asarray(vis[gfoff[g]:gfoff[g + 1]], np.float64)
            with np.errstate(all="ignore"):
                inside = (lo <= v) & (v <= hi)               # (a NaN is in no window)
            vis_counts[w, k_] += [inside.sum(), (inside & m).sum(), (inside & s).sum(),
                                  qs[inside].sum()]
    return cat_counts, vis_counts


def stage(t, frame_thr, dt_keep=None, vis=None, vis_rng=None, n_cat=None, bb_iou=None):
    """All three stages: the candidates' dict, walk()'s, cat_counts, vis_counts."""
    out = candidates(t, frame_thr, dt_keep, bb_iou)
    out.update(walk(t, out))
    out["cat_counts"], out["vis_counts"] = reduce(t, out, out["match"], out["sw"],
                                                  out["gt_clear"], vis, vis_rng, n_cat)
    return out


def table(t, frame_thr, dt_keep=None, vis=None, vis_rng=None, n_cat=None):
    """The class layer's int64[K, 11]: the identity's four frame counts, then
    cat_counts; and vis_counts."""
    s = stage(t, frame_thr, dt_keep, vis, vis_rng, n_cat)
    return np.concatenate([frame_counts(t, dt_keep, n_cat), s["cat_counts"]], 1), s


def ratios(cc):
    """The class layer's arithmetic on int64[..., 11]: dict of float64 arrays."""
    cc = np.asarray(cc, np.int64)
    gt_tracks, gt_frames, dt_frames = cc[..., 0], cc[..., 1], cc[..., 3]
    tp, idsw, motp = cc[..., 4], cc[..., 5], cc[..., 10].astype(np.float64) / ONE
    fn, fp = gt_frames - tp, dt_frames - tp
    g = np.maximum(1, tp + fn).astype(np.float64)
    tr = np.maximum(1, gt_tracks).astype(np.float64)
    out = {"mota": (tp - fp - idsw) / g, "motp": motp / np.maximum(1, tp),
           "moda": (tp - fp) / g, "smota": (motp - fp - idsw) / g, "clr_re": tp / g,
           "clr_pr": tp / np.maximum(1, tp + fp).astype(np.float64),
           "clr_f1": tp / np.maximum(1, 2 * tp + fn + fp).astype(np.float64) * 2,
           "mtr": cc[..., 7] / tr, "ptr": cc[..., 8] / tr, "mlr": cc[..., 9] / tr}
    return out


# ---------------------------------------------------------------------------
# the float statement
# ---------------------------------------------------------------------------
def clear_float(t, frame_thr, dt_keep=None, n_cat=None):
    """From the definition only, in float64: dict(cat int64[K, 6] = tp, idsw, frag,
    mt, pt, ml; motp_sum float64[K]; pairs {(cell, p): sorted (in-cell d, in-cell
    g)}; margin: the least gap between the best and the second best assignment
    of a step, over min(G, D) of the step, by enumeration; skipped: the steps too
    large for that)."""
    from itertools import permutations

    from scipy.optimize import linear_sum_assignment
    n_cat = len(t.cat_ids) if n_cat is None else n_cat
    g_off = np.asarray(t.cell_gt_off, np.int64)
    gfoff = np.asarray(t.gt_frame_off, np.int64)
    elig = _eligible(t)
    cat, motp = np.zeros((n_cat, 6), np.int64), np.zeros(n_cat)
    pairs, margins, skipped = {}, [], 0
    state = {}
    for cell, p, gl, _, dl, _, S in frame_groups(t, dt_keep):
        if not len(dl):
            continue                                         # no step
        st = state.setdefault(cell, dict(prev={}, last={}, matched={}, idsw={}, started={}))
        sim = cs(S).T                                        # [g, d]
        with np.errstate(all="ignore"):
            ok = S.T >= frame_thr
        cont = np.array([[st["prev"].get(int(g), -1) == int(d) for d in dl] for g in gl])
        score = np.where(ok & (sim > 0), 1000.0 * cont + sim, 0.0)
        r, c_ = linear_sum_assignment(-score)
        on = score[r, c_] > 0
        r, c_ = r[on], c_[on]
        if min(score.shape) <= 4 and max(score.shape) <= 6 and min(score.shape) > 0:
            # the margin of the optimum, by enumeration on small steps
            tall = score if score.shape[0] <= score.shape[1] else score.T
            sums = {}
            for pm in permutations(range(tall.shape[1]), tall.shape[0]):
                key = frozenset((i, j) for i, j in enumerate(pm) if tall[i, j] > 0)
                sums[key] = float(sum(tall[i, j] for i, j in key))
            top = sorted(sums.values())
            if len(top) > 1:
                margins.append((top[-1] - top[-2]) / min(score.shape))
        else:
            skipped += 1
        pairs[(cell, p)] = sorted(zip(dl[c_].tolist(), gl[r].tolist()))
        now = {}
        for i, j in zip(r, c_):
            g, d = int(gl[i]), int(dl[j])
            now[g] = d
            if st["last"].get(g, -1) not in (-1, d):
                st["idsw"][g] = st["idsw"].get(g, 0) + 1
            st["last"][g] = d
            st["matched"][g] = st["matched"].get(g, 0) + 1
            st["started"][g] = st["started"].get(g, 0) + (g not in st["prev"])
            k = int(t.gt_cat[g_off[cell] + g])
            if 0 <= k < n_cat:
                motp[k] += sim[i, j]
        st["prev"] = now
    for cell in range(len(g_off) - 1):
        st = state.get(cell, dict(matched={}, idsw={}, started={}))
        for g in range(g_off[cell], g_off[cell + 1]):
            k = int(t.gt_cat[g])
            if not elig[g] or not 0 <= k < n_cat:
                continue
            o = int(g - g_off[cell])
            L, m = int(gfoff[g + 1] - gfoff[g]), st["matched"].get(o, 0)
            ratio = m / L if L else 0.0
            mt, ml = ratio > 0.8, ratio < 0.2                # (TrackEval's thresholds)
            cat[k] += [m, st["idsw"].get(o, 0), max(st["started"].get(o, 0) - 1, 0),
                       mt, not mt and not ml, ml]
    return dict(cat=cat, motp_sum=motp, pairs=pairs, margins=margins, skipped=skipped)


def fixed_pairs(want, t):
    """{(cell, p): sorted (in-cell d, in-cell g)} of walk()'s steps."""
    frame_gt = np.repeat(np.arange(len(t.gt_frame_off) - 1), np.diff(t.gt_frame_off))
    g_off = np.asarray(t.cell_gt_off, np.int64)
    out = {}
    for cell, p, gf, cols, _, _, pr, _ in want["steps"]:
        out[(cell, p)] = sorted((int(cols[j]), int(frame_gt[gf[i]] - g_off[cell])) for i, j in pr)
    return out


# ---------------------------------------------------------------------------
# a seeded population whose steps are contested
# ---------------------------------------------------------------------------
def crowded_flat(seed, cells, length=24, n_cat=3):
    """A video per entry of cells = [(detection tracks, ground truths)], its cell
    of category v % n_cat.  The ground truths of a cell stand side by side and
    overlap (boxes of 10 x 10, 3 apart), each with holes; a detection track follows
    one of them with real-valued noise for a stretch and then moves to another, so
    that steps hold several rows and columns, bonuses are contested and ID
    switches happen; positions 9 and 10 hold no detection frame at all.  One
    ground truth in eight is ignored."""
    rng = np.random.default_rng(seed)
    dets, gts = [], []
    for v, (nd, ng) in enumerate(cells):
        for i in range(ng):
            fr = {p: [3.0 * i + float(rng.normal(0, 0.2)), 0.0, 10.0, 10.0]
                  for p in range(length) if rng.random() < 0.85}
            gts.append((v, v % n_cat, fr or {0: [3.0 * i, 0.0, 10.0, 10.0]},
                        int(rng.random() < 0.125)))
        for _ in range(nd):
            at, fr = int(rng.integers(max(ng, 1))), {}
            for p in range(length):
                if rng.random() < 0.12:
                    at = int(rng.integers(max(ng, 1)))
                if p not in (9, 10) and rng.random() < 0.8:
                    fr[p] = [3.0 * at + float(rng.normal(0, 0.7)), float(rng.normal(0, 0.7)),
                             10.0, 10.0]
            dets.append((v, v % n_cat, fr or {0: [0.0, 0.0, 10.0, 10.0]},
                         float(rng.integers(0, 20)) / 20, 0))
    f, _, _ = make_track_flat(len(cells), n_cat, dets, gts)
    return f


# ---------------------------------------------------------------------------
# The hand-written table: two categories, frame_thr = 0.5.  A ground truth's box
# is BOX unless said; SIX overlaps BOX by 0.6, HALF by 0.5 exactly.
# ---------------------------------------------------------------------------
SIX = [0, 0, 10, 6]
Q6 = 644245094                # q(0.6)
HAND_THR = 0.5
HAND_THR_ABOVE = 0.5 + 2.0 ** -52


def _at(x, positions, box=BOX):
    return {p: [box[0] + x, box[1], box[2], box[3]] for p in positions}


HAND_GTS = [
    # (a) video 0: continuity beats IoU; video 1: the same frame without the history
    (0, 0, _at(0, [0, 1]), 0),                                           # 0
    (1, 0, _at(0, [1]), 0),                                              # 1
    # (b) video 2: A, a step with a detection present but away, then B
    (2, 0, _at(0, [0, 1, 2]), 0),                                        # 2
    # (c) video 3: the same, but position 1 has no detection frame: no step
    (3, 0, _at(0, [0, 1, 2]), 0),                                        # 3
    # (d) video 4: two ground truths whose followers would swap on IoU alone
    (4, 0, _at(0, [0, 1]), 0),                                           # 4
    (4, 0, _at(0, [0, 1], SIX), 0),                                      # 5
    # (e) video 5: the second ground truth is absent at step 1
    (5, 0, _at(0, [0, 1, 2]), 0),                                        # 6
    (5, 0, _at(50, [0, 2]), 0),                                          # 7
    # (f) video 6, category 1: 4 of 5, 1 of 5, 0 of 5, 5 of 6 frames matched
    (6, 1, _at(0, range(5)), 0),                                         # 8
    (6, 1, _at(100, range(5)), 0),                                       # 9
    (6, 1, _at(200, range(5)), 0),                                       # 10
    (6, 1, _at(300, range(6)), 0),                                       # 11
    # (g, h) video 7: an eligible and an ignored ground truth
    (7, 1, _at(0, [0, 1]), 0),                                           # 12
    (7, 1, {p: AWAY for p in range(2)}, GT_IGNORE),                      # 13
    # (i) video 9: category 1 on the cell tables, a category outside the table in gt_cat
    (9, 1, _at(0, [0, 1]), 0),                                           # 14
]
HAND_DETS = [
    (0, 0, _at(0, [0, 1], SIX), 0.9, 0),                                 # 0  A
    (0, 0, _at(0, [1]), 0.8, 0),                                         # 1  B
    (1, 0, _at(0, [1], SIX), 0.9, 0),                                    # 2  A'
    (1, 0, _at(0, [1]), 0.8, 0),                                         # 3  B'
    (2, 0, {0: BOX, 1: AWAY}, 0.9, 0),                                   # 4
    (2, 0, _at(0, [2]), 0.8, 0),                                         # 5
    (3, 0, _at(0, [0, 2], SIX), 0.9, 0),                                 # 6
    (3, 0, _at(0, [2]), 0.8, 0),                                         # 7
    (4, 0, {0: BOX, 1: SIX}, 0.9, 0),                                    # 8
    (4, 0, {0: SIX, 1: BOX}, 0.8, 0),                                    # 9
    (5, 0, _at(0, [0, 1, 2]), 0.9, 0),                                   # 10
    (5, 0, _at(50, [0, 2]), 0.8, 0),                                     # 11
    (6, 1, _at(0, range(4)), 0.9, 0),                                    # 12
    (6, 1, _at(100, [2]), 0.8, 0),                                       # 13
    (6, 1, _at(300, range(5)), 0.7, 0),                                  # 14
    # E overlaps ground truth 12 at exactly 0.5 on frame 0
    (7, 1, {0: HALF, 1: BOX}, 0.7, 0),                                   # 15 E
    # F would win both frames: it is set aside (dt_keep = 0), as is H on the ignored one
    (7, 1, _at(0, [0, 1]), 0.9, 0),                                      # 16 F
    (7, 1, {p: AWAY for p in range(2)}, 0.8, 0),                         # 17 H
    # (i) video 8: a cell without ground truth
    (8, 1, _at(0, range(3)), 0.9, 0),                                    # 18
    (9, 1, _at(0, [0, 1]), 0.9, 0),                                      # 19
]
HAND_SET_ASIDE = [16, 17]
# per ground-truth frame in the order given: the detection given or -1, the switch flag
HAND_MATCH = [0, 0, 3, 4, -1, 5, 6, -1, 6, 8, 8, 9, 9, 10, 10, 10, 11, 11,
              12, 12, 12, 12, -1, -1, -1, 13, -1, -1, -1, -1, -1, -1, -1,
              14, 14, 14, 14, 14, -1, 15, 15, -1, -1, 19, 19]
HAND_SW = [0] * 5 + [1] + [0] * 39
HAND_GT_CLEAR = [[2, 2, 0, 1], [1, 1, 0, 1], [3, 2, 1, 2], [3, 2, 0, 1], [2, 2, 0, 1],
                 [2, 2, 0, 1], [3, 3, 0, 1], [2, 2, 0, 2], [5, 4, 0, 1], [5, 1, 0, 1],
                 [5, 0, 0, 0], [6, 5, 0, 1], [2, 2, 0, 1], [0, 0, 0, 0], [2, 2, 0, 1]]
# gt_tracks, gt_frames, dt_tracks, dt_frames, tp, idsw, frag, mt, pt, ml, motp_sum
HAND_CAT_COUNTS = [[8, 18, 12, 20, 16, 1, 2, 6, 2, 0, 10 * ONE + 6 * Q6],
                   [5, 23, 5, 15, 12, 0, 0, 2, 2, 1, 11 * ONE + ONE // 2]]
# above the threshold E's frame 0 is no candidate: ground truth 12 has 1 of 2
HAND_CAT_COUNTS_ABOVE = [HAND_CAT_COUNTS[0], [5, 23, 5, 15, 11, 0, 0, 1, 3, 1, 11 * ONE]]
HAND_MOTA = [(16 - 4 - 1) / 18, (12 - 3 - 0) / 23]
# (j) the windows overlap at 0.5; visibilities are 1 but for ground truth 2 (1, 0.2,
# 0.5: the switch lies in both halves) and frame 1 of ground truth 0 (a NaN: in none)
HAND_VIS_RNG = [[0, 1], [0, 0.5], [0.5, 1]]
HAND_VIS = {0: {1: float("nan")}, 2: {1: 0.2, 2: 0.5}}
HAND_VIS_COUNTS = [[[17, 15, 1, 10 * ONE + 5 * Q6], [23, 12, 0, 11 * ONE + ONE // 2]],
                   [[2, 1, 1, ONE], [0, 0, 0, 0]],
                   [[16, 15, 1, 10 * ONE + 5 * Q6], [23, 12, 0, 11 * ONE + ONE // 2]]]


def hand_flat():
    """(flat, dt_at, gt_at, dt_keep, vis)."""
    f, dt_at, gt_at = make_track_flat(10, 2, HAND_DETS, HAND_GTS)
    f.gt_cat = np.array(f.gt_cat)
    f.dt_cat = np.array(f.dt_cat)
    f.gt_cat[gt_at[14]] = 7
    f.dt_cat[dt_at[19]] = 7
    keep = np.ones(len(HAND_DETS), np.uint8)
    keep[dt_at[HAND_SET_ASIDE]] = 0
    vis = np.ones(len(f.gt_frame_pos))
    for i, per in HAND_VIS.items():
        s = int(f.gt_frame_off[gt_at[i]])
        for j, p in enumerate(sorted(HAND_GTS[i][2])):
            if p in per:
                vis[s + j] = per[p]
    return f, dt_at, gt_at, keep, vis


def by_given(t, dt_at, gt_at, values, rows=False):
    """Per ground-truth frame in the order the ground truths were given: `values`
    as they are, or (rows=True) in-cell rows as the numbers of the detections given."""
    d_inv = {int(r): i for i, r in enumerate(dt_at)}
    gfoff, d_off = np.asarray(t.gt_frame_off), np.asarray(t.cell_dt_off)
    out = []
    for g in gt_at:
        for k in range(gfoff[g], gfoff[g + 1]):
            v = int(values[k])
            out.append(d_inv[int(d_off[t.gt_cell[g]]) + v] if rows and v >= 0 else v)
    return out
