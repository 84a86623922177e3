"""numpy restatement of the error impact (the definition in
include/tao_amodal_hip.h, section "error impact").  TEST INFRASTRUCTURE ONLY.

Every variant's list is built explicitly, sorted with ``np.argsort(-score,
kind="mergesort")`` and swept with the reference's accumulate arithmetic
(lvis_amodal/eval.py:370-417), so every comparison against the device is ``==``.
Types, s, o and the same-category argmax come from error_types_ref."""
import numpy as np

import error_types_ref as et
import orclib

FIXES = ("BASE", "CLS", "LOC", "BOTH", "DUP", "BKG", "MISS", "FP", "FN")
BASE, F_CLS, F_LOC, F_BOTH, F_DUP, F_BKG, F_MISS, F_FP, F_FN = range(9)


def pr_at_recall(tps, num_gt, rec_thrs):
    """The reference's loop body for one IoU threshold: tps = the list's
    true-positive flags in sweep order (every other row a false positive)."""
    tps = np.asarray(tps, dtype=bool)
    tp = np.cumsum(tps).astype(dtype=float)
    fp = np.cumsum(~tps).astype(dtype=float)
    rc = tp / num_gt
    pr = tp / (fp + tp + np.spacing(1))
    # the reference's loop `if pr[i] > pr[i - 1]: pr[i - 1] = pr[i]` from the
    # right: the running maximum, the same doubles
    pr = np.maximum.accumulate(pr[::-1])[::-1].tolist()
    idx = np.searchsorted(rc, rec_thrs, side="left")
    out = [0.0] * len(rec_thrs)
    try:
        for j, pi in enumerate(idx):
            out[j] = pr[pi]
    except IndexError:
        pass
    return np.array(out)


def better(s, best):
    """A row of score s beats the holder of score `best` (a lower table row)."""
    return not np.isnan(s) and (np.isnan(best) or s > best)


def other_links(f, gt_rng, n_rng=6):
    """link_other[n_dt, n_rng]: the argmax row of o, the rule of the
    same-category argmax of error_types_ref.error_types on the other categories."""
    n_dt = int(f.cell_dt_off[-1])
    dt_cat, gt_cat = np.asarray(f.dt_cat), np.asarray(f.gt_cat)
    dt_box = np.asarray(f.dt_box, dtype=np.float64).reshape(-1, 4)
    gt_box = np.asarray(f.gt_box, dtype=np.float64).reshape(-1, 4)
    gt_rng = np.asarray(gt_rng).astype(np.uint32)
    d_img, g_img = et.units(f)
    link = -np.ones((n_dt, n_rng), dtype=np.int64)
    for u in np.unique(d_img):
        D = np.flatnonzero(d_img == u)
        G = np.flatnonzero(g_img == u)
        if len(G) == 0:
            continue
        iou = orclib.bb_iou(dt_box[D], gt_box[G])
        iou = np.where(np.isnan(iou), -1.0, iou)
        same = dt_cat[D][:, None] == gt_cat[G][None, :]
        for a in range(n_rng):
            ev = ((gt_rng[G] >> np.uint32(a)) & 1) == 0
            oth = np.where(~same & ev[None, :], iou, -1.0)
            link[D, a] = np.where(oth.max(1) >= 0, G[oth.argmax(1)], -1)
    return link


def impact_tables(n_cat, n_rng, dt_cat, score, dt_type, link_same, link_other, gt_cat, gt_rng,
                  held, rec_thrs):
    """The definition on bare tables.  Returns dict(precision float64[9, R, K,
    n_rng], num_gt int64[9, K, n_rng], events: counts of what happened)."""
    dt_cat, gt_cat = np.asarray(dt_cat, dtype=np.int64), np.asarray(gt_cat, dtype=np.int64)
    score = np.asarray(score, dtype=np.float64)
    gt_rng = np.asarray(gt_rng).astype(np.uint32)
    held = np.asarray(held).astype(bool)
    links = (np.asarray(link_same), np.asarray(link_other))
    n_gt, R = len(gt_cat), len(rec_thrs)
    P = -np.ones((9, R, n_cat, n_rng))
    NG = np.zeros((9, n_cat, n_rng), dtype=np.int64)
    events = dict(winner=0, lost_to_held=0, lost_to_better=0, adopted=0, unlinked_missed=0,
                  linked_missed=0)
    rows_of = [np.flatnonzero(dt_cat == c) for c in range(n_cat)]
    for a in range(n_rng):
        ty_a = np.asarray(dt_type)[:, a]
        ev = ((gt_rng >> np.uint32(a)) & 1) == 0
        missed = ev & ~held[a]
        win = ({}, {})
        for tab, t in ((0, et.LOC), (1, et.CLS)):
            for d in np.flatnonzero(ty_a == t):              # table rows ascending
                g = int(links[tab][d, a])
                if g < 0 or g >= n_gt:
                    continue
                if held[a, g]:
                    events["lost_to_held"] += 1
                    continue
                cur = win[tab].get(g)
                if cur is None:
                    win[tab][g] = int(d)
                else:
                    events["lost_to_better"] += 1
                    if better(score[d], score[cur]):
                        win[tab][g] = int(d)
        events["winner"] += len(win[0]) + len(win[1])
        linked = np.zeros(n_gt, dtype=bool)
        linked[list(win[0]) + list(win[1])] = True
        events["unlinked_missed"] += int((missed & ~linked).sum())
        events["linked_missed"] += int((missed & linked).sum())
        adopted = [[] for _ in range(n_cat)]
        for g, d in win[1].items():
            adopted[gt_cat[g]].append(score[d])
            events["adopted"] += 1
        loc_winner = np.zeros(len(dt_cat), dtype=bool)
        loc_winner[list(win[0].values())] = True
        for c in range(n_cat):
            rows = rows_of[c]
            ty, sc = ty_a[rows], score[rows]
            kept = (ty == et.TP) | ((ty >= et.DUP) & (ty <= et.BKG))
            tp = ty == et.TP
            n_ev = int((ev & (gt_cat == c)).sum())
            n_missed = int((missed & (gt_cat == c)).sum())
            n_unlinked = int((missed & ~linked & (gt_cat == c)).sum())

            def run(v, keep, tps, ng, extra=()):
                NG[v, c, a] = ng
                if ng <= 0:
                    return
                s = np.concatenate([sc[keep], np.asarray(extra, dtype=np.float64)])
                t = np.concatenate([tps[keep], np.ones(len(extra), dtype=bool)])
                o = np.argsort(-s, kind="mergesort")
                P[v, :, c, a] = pr_at_recall(t[o], ng, rec_thrs)

            run(BASE, kept, tp, n_ev)
            run(F_CLS, kept & (ty != et.CLS), tp, n_ev, adopted[c])
            lk = links[0][rows, a]
            linkd = (ty == et.LOC) & (lk >= 0) & (lk < n_gt)
            to_held = np.zeros(len(rows), dtype=bool)
            to_held[linkd] = held[a, lk[linkd]]
            wins = linkd & ~to_held & loc_winner[rows]
            run(F_LOC, kept & ~(linkd & ~wins), tp | wins, n_ev)
            run(F_BOTH, kept & (ty != et.BOTH), tp, n_ev)
            run(F_DUP, kept & (ty != et.DUP), tp, n_ev)
            run(F_BKG, kept & (ty != et.BKG), tp, n_ev)
            run(F_MISS, kept, tp, n_ev - n_unlinked)
            run(F_FP, tp, tp, n_ev)
            run(F_FN, kept, tp, n_ev - n_missed)
    return dict(precision=P, num_gt=NG, events=events)


def error_impact(f, match_gt, gt_rng, iou_thrs, slot, tb, n_rng=6, rec_thrs=None):
    """The impact on a Flat of the image level: error_types_ref.error_types for
    the types and the same-category links, other_links, then impact_tables.
    Adds link_same, link_other, held and the breakdown itself ("types")."""
    if rec_thrs is None:
        rec_thrs = orclib.thresholds()[1]
    e = et.error_types(f, match_gt, gt_rng, iou_thrs, slot, tb, n_rng)
    link_other = other_links(f, gt_rng, n_rng)
    out = impact_tables(len(f.cat_ids), n_rng, f.dt_cat, f.dt_score, e["dt_type"], e["arg"],
                        link_other, f.gt_cat, gt_rng, e["hit"], rec_thrs)
    out.update(link_same=e["arg"], link_other=link_other, held=e["hit"], types=e)
    return out


def sweep_order(dt_cat, score, n_cat):
    """(cat_off int32[n_cat + 1], order int32[n_dt]): per category the table
    rows by stable descending score, NaN last -- what the device sort leaves."""
    dt_cat, score = np.asarray(dt_cat), np.asarray(score, dtype=np.float64)
    off = np.zeros(n_cat + 1, dtype=np.int32)
    np.cumsum(np.bincount(dt_cat, minlength=n_cat), out=off[1:])
    parts = []
    for c in range(n_cat):
        rows = np.flatnonzero(dt_cat == c)
        parts.append(rows[np.argsort(-score[rows], kind="mergesort")])
    order = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return off, order.astype(np.int32)
