"""numpy restatement of the image-level error breakdown (the definition in
include/tao_amodal_hip.h, section "image-level error breakdown per range").
TEST INFRASTRUCTURE ONLY.

IoUs come from the C oracle's bbIou (orclib.bb_iou), the arithmetic of the
kernel's box_iou, so every comparison against the device is ``==``."""
import numpy as np

import orclib

TYPES = ("TP", "IGNORED", "DUP", "LOC", "CLS", "BOTH", "BKG")
TP, IGNORED, DUP, LOC, CLS, BOTH, BKG = range(7)
DT_IGNORE_UNMATCHED = 1
N_THR = 10


def foreground(iou_thrs, slot):
    """tf of a slot: the clamp the match uses."""
    return min(float(np.asarray(iou_thrs)[slot]), 1 - 1e-10)


def units(f):
    """(image of every detection row, image of every ground-truth row)."""
    cell_unit = np.asarray(f.cell_unit, dtype=np.int64)
    g_cell = np.repeat(np.arange(f.n_cells), np.diff(np.asarray(f.cell_gt_off)))
    d_cell = np.repeat(np.arange(f.n_cells), np.diff(np.asarray(f.cell_dt_off)))
    return cell_unit[d_cell], cell_unit[g_cell]


def error_types(f, match_gt, gt_rng, iou_thrs, slot, tb, n_rng=6):
    """f: a Flat of the image level (use_cats = 1); match_gt[n_dt, n_rng * 10]:
    in-cell index of the matched ground truth or -1 per (range, threshold);
    gt_rng[n_gt]: bit a set = ignored in range a.  Returns dict(dt_type
    uint8[n_dt, n_rng], dt_counts int64[n_rng, K, 7], gt_counts int64[n_rng, K,
    3], s, o float64[n_dt, n_rng], arg int64[n_dt, n_rng] (the same-category
    argmax row or -1), hit bool[n_rng, n_gt])."""
    tf = foreground(iou_thrs, slot)
    assert 0 <= tb < tf
    n_dt, n_gt = int(f.cell_dt_off[-1]), int(f.cell_gt_off[-1])
    K = len(f.cat_ids)
    dt_cat, gt_cat = np.asarray(f.dt_cat), np.asarray(f.gt_cat)
    dt_box = np.asarray(f.dt_box, dtype=np.float64).reshape(-1, 4)
    gt_box = np.asarray(f.gt_box, dtype=np.float64).reshape(-1, 4)
    flags = np.asarray(f.dt_flags)
    gt_rng = np.asarray(gt_rng).astype(np.uint32)
    d_cell = np.repeat(np.arange(f.n_cells), np.diff(np.asarray(f.cell_dt_off)))
    gt0 = np.asarray(f.cell_gt_off)[d_cell].astype(np.int64)
    d_img, g_img = units(f)
    match_gt = np.asarray(match_gt).reshape(n_dt, -1)

    s = np.zeros((n_dt, n_rng))
    o = np.zeros((n_dt, n_rng))
    arg = -np.ones((n_dt, n_rng), dtype=np.int64)
    for u in np.unique(d_img):
        D = np.flatnonzero(d_img == u)
        G = np.flatnonzero(g_img == u)            # rows ascending
        if len(G) == 0:
            continue
        iou = orclib.bb_iou(dt_box[D], gt_box[G])
        iou = np.where(np.isnan(iou), -1.0, iou)   # a NaN overlap is no overlap
        same = dt_cat[D][:, None] == gt_cat[G][None, :]
        for a in range(n_rng):
            ev = ((gt_rng[G] >> np.uint32(a)) & 1) == 0
            own = np.where(same & ev[None, :], iou, -1.0)
            oth = np.where(~same & ev[None, :], iou, -1.0)
            best = own.max(1)
            has = best >= 0
            s[D, a] = np.where(has, best, 0.0)
            arg[D, a] = np.where(has, G[own.argmax(1)], -1)   # first = lowest row
            o[D, a] = np.maximum(oth.max(1), 0.0)

    dt_type = np.full((n_dt, n_rng), BKG, dtype=np.uint8)
    hit = np.zeros((n_rng, n_gt), dtype=bool)
    loc = np.zeros((n_rng, n_gt), dtype=bool)
    for a in range(n_rng):
        m = match_gt[:, a * N_THR + slot].astype(np.int64)
        matched = m >= 0
        grow = np.where(matched, gt0 + m, 0)
        g_ign = np.zeros(n_dt, dtype=bool)
        if n_gt:
            g_ign = ((gt_rng[grow] >> np.uint32(a)) & 1) == 1
        un = ~matched
        t = np.full(n_dt, BKG, dtype=np.uint8)
        t[un & (o[:, a] >= tb)] = BOTH
        t[un & (o[:, a] >= tf)] = CLS
        t[un & (s[:, a] >= tb)] = LOC
        t[un & (s[:, a] >= tf)] = DUP
        t[un & ((flags & DT_IGNORE_UNMATCHED) != 0)] = IGNORED
        t[matched] = np.where(g_ign[matched], IGNORED, TP)
        dt_type[:, a] = t
        hit[a, grow[matched]] = True
        at = arg[t == LOC, a]
        loc[a, at[at >= 0]] = True

    dt_counts = np.zeros((n_rng, K, 7), dtype=np.int64)
    gt_counts = np.zeros((n_rng, K, 3), dtype=np.int64)
    for a in range(n_rng):
        np.add.at(dt_counts[a], (dt_cat, dt_type[:, a]), 1)
        ev = ((gt_rng >> np.uint32(a)) & 1) == 0
        np.add.at(gt_counts[a, :, 0], gt_cat[ev], 1)
        np.add.at(gt_counts[a, :, 1], gt_cat[ev & ~hit[a]], 1)
        np.add.at(gt_counts[a, :, 2], gt_cat[ev & ~hit[a] & loc[a]], 1)
    return dict(dt_type=dt_type, dt_counts=dt_counts, gt_counts=gt_counts,
                s=s, o=o, arg=arg, hit=hit)


def make_flat(n_img, n_cat, dets, gts):
    """A hand-made image-level Flat.  dets: (image, category, box, score, flags),
    gts: (image, category, box, visibility, flags).  Category-major cells like
    flatten.flatten_lvis: a cell's detections by descending score (stable), its
    ground truths in the order given.  Returns (flat, dt_at, gt_at): the table
    row of the i-th detection / ground truth given."""
    from tao_amodal_amd.flatten import Flat
    I32 = np.int32
    d_key = np.array([c * n_img + u for u, c, _, _, _ in dets], dtype=np.int64)
    g_key = np.array([c * n_img + u for u, c, _, _, _ in gts], dtype=np.int64)
    d_score = np.array([d[3] for d in dets], dtype=np.float64)
    d_ord = np.lexsort((np.arange(len(dets)), -d_score, d_key)) if len(dets) \
        else np.zeros(0, np.int64)
    g_ord = np.argsort(g_key, kind="stable") if len(gts) else np.zeros(0, np.int64)
    keys = np.unique(np.concatenate([d_key, g_key]))
    f = Flat()
    f.kind, f.use_cats = "lvis", True
    f.img_ids = np.arange(n_img, dtype=np.int64)
    f.cat_ids = np.arange(n_cat, dtype=np.int64)
    f.n_cells = len(keys)
    f.cell_unit = (keys % n_img).astype(I32)
    f.cell_cat = (keys // n_img).astype(I32)
    f.cell_dt_off = np.searchsorted(d_key[d_ord], np.r_[keys, np.inf]).astype(I32)
    f.cell_gt_off = np.searchsorted(g_key[g_ord], np.r_[keys, np.inf]).astype(I32)
    f.dt_box = np.array([dets[i][2] for i in d_ord], dtype=np.float64).reshape(-1, 4)
    f.dt_row = d_ord.astype(np.int64)
    f.dt_score = np.ascontiguousarray(d_score[d_ord])
    f.dt_flags = np.array([dets[i][4] for i in d_ord], dtype=np.uint8)
    f.dt_id = d_ord.astype(np.int64) + 1
    f.dt_cat = (d_key[d_ord] // n_img).astype(I32)
    f.dt_cell = np.searchsorted(keys, d_key[d_ord]).astype(I32)
    f.gt_box = np.array([gts[i][2] for i in g_ord], dtype=np.float64).reshape(-1, 4)
    f.gt_row = g_ord.astype(np.int64)
    f.gt_vis = np.array([gts[i][3] for i in g_ord], dtype=np.float64)
    f.gt_flags = np.array([gts[i][4] for i in g_ord], dtype=np.uint8)
    f.gt_id = g_ord.astype(np.int64) + 1
    f.gt_cat = (g_key[g_ord] // n_img).astype(I32)
    f.gt_cell = np.searchsorted(keys, g_key[g_ord]).astype(I32)
    f.n_pairs = int(np.sum(np.diff(f.cell_dt_off).astype(np.int64) * np.diff(f.cell_gt_off)))
    dt_at = np.empty(len(dets), dtype=np.int64)
    dt_at[d_ord] = np.arange(len(dets))
    gt_at = np.empty(len(gts), dtype=np.int64)
    gt_at[g_ord] = np.arange(len(gts))
    return f, dt_at, gt_at


# ---------------------------------------------------------------------------
# The hand-written table: tf = 0.5 (slot 0), tb = 0.125.  Ground truths are
# fully visible: evaluated in ranges 0 ("all") and 3, ignored in 1, 2, 4 and 5.
# ---------------------------------------------------------------------------
HAND_TB = 0.125
HAND_GTS = [
    # image 0: one detection of each type
    (0, 0, [0, 0, 10, 10], 1.0, 0),      # 0  held by the TP
    (0, 0, [100, 0, 10, 10], 1.0, 1),    # 1  "ignore": holds the IGNORED detection
    (0, 0, [200, 0, 10, 10], 1.0, 0),    # 2  missed, with a LOC neighbour
    (0, 1, [300, 0, 10, 10], 1.0, 0),    # 3  missed, without one
    # image 1: IoU exactly at tf and exactly at tb
    (1, 0, [0, 0, 1, 1], 1.0, 0),        # 4
    (1, 0, [10, 0, 4, 2], 1.0, 0),       # 5  missed, LOC neighbour at exactly tb
    # image 2: two ground truths at the same IoU
    (2, 0, [0, 0, 10, 10], 1.0, 0),      # 6  missed; the LOC row's argmax: the lower row
    (2, 0, [0, 0, 10, 10], 1.0, 0),      # 7  held: were it the argmax, missed_loc would be 2
]
HAND_DETS = [
    (0, 0, [0, 0, 10, 10], 0.9, 0),      # 0  TP: IoU 1 with gt 0
    (0, 0, [100, 0, 10, 10], 0.8, 0),    # 1  IGNORED: matched to the ignored gt 1
    (0, 0, [0, 0, 10, 9], 0.7, 0),       # 2  DUP: IoU 0.9 with gt 0, which is taken
    (0, 0, [200, 0, 10, 3], 0.6, 0),     # 3  LOC: IoU 0.3 with gt 2
    (0, 0, [300, 0, 10, 10], 0.5, 0),    # 4  CLS: IoU 1 with gt 3 of category 1
    (0, 0, [300, 0, 10, 2], 0.4, 0),     # 5  BOTH: IoU 0.2 with gt 3
    (0, 0, [500, 0, 10, 10], 0.3, 0),    # 6  BKG
    (1, 0, [0, 0, 2, 1], 0.9, 0),        # 7  TP: IoU exactly 0.5 with gt 4
    (1, 0, [0, 0, 2, 1], 0.8, 0),        # 8  DUP: s == tf
    (1, 0, [10, 0, 1, 1], 0.7, 0),       # 9  LOC: 1 / 8 == tb with gt 5
    (1, 1, [0, 0, 2, 1], 0.6, 0),        # 10 CLS: o == tf
    (1, 1, [10, 0, 1, 1], 0.5, 0),       # 11 BOTH: o == tb
    (1, 2, [50, 50, 5, 5], 0.4, 1),      # 12 IGNORED: unmatched, not-exhaustive
    (2, 0, [0, 0, 10, 3], 0.9, 0),       # 13 LOC: IoU 0.3 with gt 6 and gt 7
    (2, 0, [0, 0, 10, 10], 0.95, 0),     # 14 TP: IoU 1 with both, the match takes the LATER, gt 7
]
# type of every detection above in range 0, and in range 1 (no ground truth is
# evaluated: a match is to an ignored one, nothing else overlaps anything)
HAND_TYPES_RNG0 = [0, 1, 2, 3, 4, 5, 6, 0, 2, 3, 4, 5, 1, 3, 0]
HAND_TYPES_RNG1 = [1, 1, 6, 6, 6, 6, 6, 1, 6, 6, 6, 6, 1, 6, 1]
# range 0: dt_counts[category][type], gt_counts[category] = evaluated, missed, missed_loc
HAND_DT_COUNTS_RNG0 = [[3, 1, 2, 3, 1, 1, 1], [0, 0, 0, 0, 1, 1, 0], [0, 1, 0, 0, 0, 0, 0]]
HAND_GT_COUNTS_RNG0 = [[6, 3, 3], [1, 1, 0], [0, 0, 0]]


def hand_flat():
    return make_flat(3, 3, HAND_DETS, HAND_GTS)
