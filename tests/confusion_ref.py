"""numpy restatement of the confusion (the definition in
include/tao_amodal_hip.h, section "confusion").  TEST INFRASTRUCTURE ONLY.

A loop over (row, range) into a dict keyed (a, c, c'); the winners by
error_impact_ref.better, rows ascending.  Every value is an integer: every
comparison against the device is ``==``."""
import numpy as np

import error_types_ref as et
from error_impact_ref import better

COLUMNS = ("cls", "both", "unheld", "adopted")
I_CLS, I_BOTH, I_UNHELD, I_ADOPTED = range(4)


def segments(dt_cat, n_cat):
    """cat_off int32[n_cat + 1] of a category-major table."""
    dt_cat = np.asarray(dt_cat, dtype=np.int64)
    assert (np.diff(dt_cat) >= 0).all(), "the rows lie category-major"
    off = np.zeros(n_cat + 1, dtype=np.int32)
    np.cumsum(np.bincount(dt_cat, minlength=n_cat), out=off[1:])
    return off


def confusion_tables(n_cat, n_rng, cat_off, score, dt_cat, dt_type, link_other, gt_cat, held):
    """The definition on bare tables: {(a, c, c'): [cls, both, unheld, adopted]}."""
    dt_cat, gt_cat = np.asarray(dt_cat, dtype=np.int64), np.asarray(gt_cat, dtype=np.int64)
    score = np.asarray(score, dtype=np.float64)
    n_dt, n_gt = len(dt_cat), len(gt_cat)
    dt_type = np.asarray(dt_type).reshape(n_dt, n_rng)
    link = np.asarray(link_other).reshape(n_dt, n_rng)
    held = np.asarray(held).reshape(n_rng, n_gt).astype(bool)
    off = np.clip(np.asarray(cat_off, dtype=np.int64), 0, n_dt)
    seg = -np.ones(n_dt, dtype=np.int64)              # the segment a row lies in
    for c in range(n_cat):
        seg[off[c]:max(off[c + 1], off[c])] = c
    pairs = {}
    for a in range(n_rng):
        # the impact's winners: the CLS rows of every category in [0, n_cat)
        win = {}
        for d in range(n_dt):
            g = int(link[d, a])
            if not 0 <= dt_cat[d] < n_cat or dt_type[d, a] != et.CLS or not 0 <= g < n_gt \
                    or held[a, g]:
                continue
            if g not in win or better(score[d], score[win[g]]):
                win[g] = d
        for d in range(n_dt):
            c, ty, g = int(dt_cat[d]), int(dt_type[d, a]), int(link[d, a])
            if seg[d] != c or ty not in (et.CLS, et.BOTH) or not 0 <= g < n_gt \
                    or not 0 <= gt_cat[g] < n_cat:
                continue
            n = pairs.setdefault((a, c, int(gt_cat[g])), [0, 0, 0, 0])
            if ty == et.BOTH:
                n[I_BOTH] += 1
                continue
            n[I_CLS] += 1
            if not held[a, g]:
                n[I_UNHELD] += 1
                n[I_ADOPTED] += win[g] == d
    return pairs


def csr(pairs, n_cat, n_rng):
    """The sparse result as the device leaves it: (ent_off int64[n_rng * n_cat + 1],
    ent_gt_cat int32[n], ent_counts int32[n, 4])."""
    keys = sorted(pairs)
    off = np.zeros(n_rng * n_cat + 1, dtype=np.int64)
    for a, c, _ in keys:
        off[a * n_cat + c + 1] += 1
    np.cumsum(off, out=off)
    return (off, np.array([k[2] for k in keys], dtype=np.int32),
            np.array([pairs[k] for k in keys], dtype=np.int32).reshape(-1, 4))


def of_impact(f, out, n_rng):
    """The pairs of a Flat from what error_impact_ref.error_impact /
    track_error_impact_ref.error_impact returned for it."""
    n_cat = len(f.cat_ids)
    return confusion_tables(n_cat, n_rng, segments(f.dt_cat, n_cat), f.dt_score, f.dt_cat,
                            out["types"]["dt_type"], out["link_other"], f.gt_cat, out["held"])


def check_invariants(pairs, n_cat, n_rng, dt_counts, adopted_into):
    """The three invariants of the definition.  dt_counts[n_rng, K, 7] of the
    breakdown; adopted_into[n_rng, K]: the rows the impact's CLS variant adopts
    into (a, c')."""
    cls = np.zeros((n_rng, n_cat), dtype=np.int64)
    both = np.zeros((n_rng, n_cat), dtype=np.int64)
    into = np.zeros((n_rng, n_cat), dtype=np.int64)
    for (a, c, c2), n in pairs.items():
        assert c != c2 and n[I_CLS] + n[I_BOTH] > 0
        assert 0 <= n[I_ADOPTED] <= n[I_UNHELD] <= n[I_CLS]
        cls[a, c] += n[I_CLS]
        both[a, c] += n[I_BOTH]
        into[a, c2] += n[I_ADOPTED]
    assert np.array_equal(cls, np.asarray(dt_counts)[:, :, et.CLS])
    assert np.array_equal(both, np.asarray(dt_counts)[:, :, et.BOTH])
    assert np.array_equal(into, np.asarray(adopted_into))


def adopted_into(f, out, n_rng):
    """[n_rng, K]: per (range, category) the CLS winners of its missed ground
    truths -- what impact_tables adopts, restated from its definition."""
    n_cat, n_gt = len(f.cat_ids), len(f.gt_cat)
    ty, link, held = out["types"]["dt_type"], out["link_other"], np.asarray(out["held"], bool)
    got = np.zeros((n_rng, n_cat), dtype=np.int64)
    for a in range(n_rng):
        rows = np.flatnonzero(ty[:, a] == et.CLS)
        g = link[rows, a]
        g = g[(g >= 0) & (g < n_gt)]
        g = np.unique(g[~held[a, g]])
        np.add.at(got[a], np.asarray(f.gt_cat)[g], 1)
    return got


def relabelled(gtj, predj):
    """The predictions with every third track handed to the next category: the
    recorded fixtures hold few classification errors, these hold many, on both
    levels (a track keeps one category)."""
    cats = sorted(c["id"] for c in gtj["categories"])
    nxt = {c: cats[(i + 1) % len(cats)] for i, c in enumerate(cats)}
    return [dict(p, category_id=nxt[p["category_id"]]) if p["track_id"] % 3 == 0 else p
            for p in predj]
