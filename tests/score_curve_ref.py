"""numpy restatement of the track-level score thresholds (the definition in
include/tao_amodal_hip.h, section "track-level score thresholds").  TEST
INFRASTRUCTURE ONLY.

A composition of the restatements that exist: the pass rule here; a layer of the
identity as identity_ref.identity_from_share on the input the header names --
the share rows of the tracks that do not pass zeroed, DT_IGNORE_UNMATCHED set in
their flags --; HOTA and CLEAR as hota_ref.stage / frame_counts and
clear_ref.table with the layer's kept column as dt_keep."""
from types import SimpleNamespace

import numpy as np

import clear_ref
import hota_ref
import identity_ref

MAX_THRS = 64


def score_pass(dt_score, dt_cat, thr, base=None):
    """uint8[n_thr, n_dt]: the pass rule, thr float64[n_thr, n_cat]."""
    score = np.asarray(dt_score, dtype=np.float64).reshape(-1)
    cat = np.asarray(dt_cat, dtype=np.int64).reshape(-1)
    thr = np.asarray(thr, dtype=np.float64)
    n_thr, n_cat = thr.shape
    assert 1 <= n_thr <= MAX_THRS
    inside = (cat >= 0) & (cat < n_cat)
    out = np.zeros((n_thr, len(score)), np.uint8)
    for t in range(n_thr):
        mine = thr[t][np.where(inside, cat, 0)]
        with np.errstate(invalid="ignore"):
            on = inside & (score >= mine)              # (a NaN compares false)
        if base is not None:
            on &= np.asarray(base).reshape(-1)[:len(score)] != 0
        out[t] = on
    return out


def edited_input(t, share, passed):
    """(table, share) with the rows of the tracks that do not pass zeroed and
    DT_IGNORE_UNMATCHED set in their flags: the input whose unthresholded
    identity IS the layer."""
    d_off, g_off = np.asarray(t.cell_dt_off, np.int64), np.asarray(t.cell_gt_off, np.int64)
    ioff = np.asarray(t.cell_iou_off, np.int64)
    n_dt = int(d_off[-1])
    passed = np.asarray(passed).reshape(-1)[:n_dt] != 0
    sh = np.array(share, dtype=np.int32)
    for c in range(len(d_off) - 1):
        D, G = int(d_off[c + 1] - d_off[c]), int(g_off[c + 1] - g_off[c])
        cell = sh[ioff[c]:ioff[c] + D * G].reshape(D, G)       # (a view)
        cell[~passed[d_off[c]:d_off[c + 1]]] = 0
    # (the columns the assignment reads, of a Flat or of identity_ref.table)
    e = SimpleNamespace(**{k: getattr(t, k) for k in (
        "cell_dt_off", "cell_gt_off", "cell_iou_off", "gt_cat", "gt_flags", "dt_cat",
        "dt_frame_off", "gt_frame_off", "cat_ids")})
    flags = np.array(np.asarray(t.dt_flags)[:n_dt], dtype=np.uint8)
    flags[~passed] |= identity_ref.DT_IGNORE_UNMATCHED
    e.dt_flags = flags
    return e, sh


def identity_layer(t, share, passed):
    """identity_ref.identity_from_share of the edited input, with "share" (the
    edited one: what check_assignment needs)."""
    e, sh = edited_input(t, share, passed)
    out = identity_ref.identity_from_share(e, sh)
    out["share"] = sh
    return out


def layer_tables(f, frame_thr, thr_row, alphas=None, share=None):
    """What identity(), hota() and clear() report at one threshold row
    (float64[n_cat], the tables' category order) on the Flat f: dict(ident: the
    identity's layer, hota: hota_ref.stage's dict with "counts" int64[K, 4], clear:
    int64[K, 11])."""
    share = identity_ref.share(f, frame_thr) if share is None else share
    passed = score_pass(f.dt_score, f.dt_cat, np.asarray(thr_row, np.float64)[None])[0]
    ident = identity_layer(f, share, passed)
    keep = ident["kept"].astype(np.uint8)
    out = {"ident": ident, "keep": keep}
    if alphas is not None:
        out["hota"] = hota_ref.stage(f, alphas, dt_keep=keep)
        out["hota"]["counts"] = hota_ref.frame_counts(f, dt_keep=keep)
    out["clear"] = clear_ref.table(f, frame_thr, dt_keep=keep)[0]
    return out


def best_index(values):
    """The first index of the greatest value that is not a NaN; -1 for none."""
    best, at = None, -1
    for i, v in enumerate(np.asarray(values, dtype=np.float64).tolist()):
        if v == v and (best is None or v > best):
            best, at = v, i
    return at
