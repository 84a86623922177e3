"""numpy restatement of the track-level error impact (the definitions in
include/tao_amodal_hip.h, sections "track-level error breakdown per range" and
"error impact").  TEST INFRASTRUCTURE ONLY.

Types, the same-category argmax and the held marks are
track_error_types_ref.error_types'; the cross-category links come from its
per-video blocks of the plan-less 3D IoU (the C oracle's arithmetic), the rule
of error_impact_ref.other_links; the nine variants are
error_impact_ref.impact_tables unchanged.  Every comparison against the device
is ``==``."""
import numpy as np

import error_impact_ref as imp
import orclib
import track_error_types_ref as te

from error_impact_ref import (BASE, FIXES, F_BKG, F_BOTH, F_CLS, F_DUP, F_FN, F_FP,  # noqa: F401
                              F_LOC, F_MISS)


def other_links(f, gt_rng, n_rng=20, dt_listed=None, gt_listed=None):
    """link_other int64[n_dt, n_rng]: the table row of the argmax of o.  A NaN
    IoU is no overlap, the argmax is the LOWEST row among equal IoUs, a best
    value below 0 (nothing evaluated, or NaNs alone) links nothing; a row the
    per-video lists leave out has no pair at all."""
    n_dt = int(f.cell_dt_off[-1])
    dt_cat, gt_cat = np.asarray(f.dt_cat), np.asarray(f.gt_cat)
    gt_rng = np.asarray(gt_rng).astype(np.uint32)
    link = -np.ones((n_dt, n_rng), dtype=np.int64)
    for D, G, iou in te.cross_blocks(f, dt_listed, gt_listed):
        # (G ascends: pooled() lists a video's rows in ascending order, so the
        # first maximum of a line is the lowest row)
        assert (np.diff(G) > 0).all()
        iou = np.where(np.isnan(iou), -1.0, iou)
        other = dt_cat[D][:, None] != gt_cat[G][None, :]
        for a in range(n_rng):
            ev = ((gt_rng[G] >> np.uint32(a)) & 1) == 0
            oth = np.where(other & ev[None, :], iou, -1.0)
            link[D, a] = np.where(oth.max(1) >= 0, G[oth.argmax(1)], -1)
    return link


def error_impact(f, iou, match_gt, gt_rng, dt_rng, iou_thrs, slot, tb, n_rng=20, rec_thrs=None,
                 dt_listed=None, gt_listed=None):
    """The impact on a Flat of the track level: track_error_types_ref.error_types
    for the types, the same-category links (`arg`) and the held marks (`hit`),
    other_links, then error_impact_ref.impact_tables.  Adds link_same,
    link_other, held and the breakdown itself ("types")."""
    if rec_thrs is None:
        rec_thrs = orclib.thresholds()[1]
    e = te.error_types(f, iou, match_gt, gt_rng, dt_rng, iou_thrs, slot, tb, n_rng,
                       dt_listed=dt_listed, gt_listed=gt_listed)
    link_other = other_links(f, gt_rng, n_rng, dt_listed, gt_listed)
    out = imp.impact_tables(len(f.cat_ids), n_rng, f.dt_cat, f.dt_score, e["dt_type"], e["arg"],
                            link_other, f.gt_cat, gt_rng, e["hit"], rec_thrs)
    out.update(link_same=e["arg"], link_other=link_other, held=e["hit"], types=e)
    return out
