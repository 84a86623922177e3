"""The analyses of TaoEval that read the track tables alone -- association(),
occlusions(), identity(), hota(), clear(), tracking_curve() -- and their text
tables: the class layer over GpuRun.association_table / occlusion_table /
identity_table / hota_table / clear_table / curve_tables.  The track
level's alone; the methods of TaoEval carry the documentation and call in here
with the evaluator `ev`."""
import numpy as np

from ... import _lib
from .._core import _params_cats


def _frame_thr(ev, frame_thr):
    """The per-frame threshold as a float in (0, 1], behind evaluate()."""
    if ev._run is None:
        raise RuntimeError("Please run evaluate() first.")
    frame_thr = float(frame_thr)
    if not 0 < frame_thr <= 1:
        raise ValueError("frame_thr: {} is not in (0, 1]".format(frame_thr))
    return frame_thr


def _cached(cache, key, make, optional):
    """make() once per key; the (key, asked) of `optional` that are not asked
    for -- the per-track tables -- are left out of what is returned."""
    hit = cache.get(key)
    if hit is None:
        hit = cache[key] = make()
    drop = [k for k, on in optional if not on]
    return {k: v for k, v in hit.items() if k not in drop}


def score_thr_of(ev, score_thr):
    """`score_thr` of identity(), hota() and clear() as None or float64[K] in the
    order of params.cat_ids: a float is every category's.  A NaN is allowed (no
    track of that category passes), so that tracking_curve()'s
    "best_per_category" can be passed back."""
    if score_thr is None:
        return None
    K = len(ev.params.cat_ids)
    try:
        a = np.asarray(score_thr, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("score_thr: {!r} is neither a float nor {} floats".format(score_thr, K))
    if a.ndim == 0:
        return np.full(K, float(a))
    if a.shape != (K,):
        raise ValueError("score_thr: {} values; a float or one per category of "
                         "params.cat_ids ({})".format(a.size, K))
    return np.ascontiguousarray(a)


def _table_thr(ev, thr):
    """Thresholds [..., K] in the order of params.cat_ids as the tables' [...,
    K_table]: a category of the tables that params.cat_ids does not name gets
    +inf (none of its tracks passes; its rows are not reported either).  None
    (no threshold) stays None."""
    if thr is None or ev._cat_pos is None or not ev.params.use_cats:
        return thr
    out = np.full(thr.shape[:-1] + (len(ev.flat.cat_ids),), np.inf)
    out[..., ev._cat_pos] = thr
    return out


def _key(thr, *parts):
    """The cache key of a result: `parts`, and the thresholds where the call had any."""
    return parts if thr is None else parts + (thr.tobytes(),)


def _with_score_thr(out, thr):
    """The result `out` with "score_thr" where the call had one."""
    if thr is not None:
        out["score_thr"] = thr
    return out


def _thr_text(thr):
    """" | score>=..." for the first line of a text table, "" without a threshold."""
    if thr is None:
        return ""
    one = len(thr) and (thr == thr[0]).all()
    return " | score>={}".format("{:g}".format(thr[0]) if one else "per category")


def _track_ids(rows, ids):
    """Table rows as the track ids `ids` of that table, -1 for none."""
    rows, ids = np.asarray(rows).astype(np.int64), np.asarray(ids, dtype=np.int64)
    if not len(ids):
        return np.full(len(rows), -1, dtype=np.int64)
    return np.where(rows >= 0, ids[np.maximum(rows, 0)], -1)


def _follower_ids(flat, cell, best):
    """In-cell followers `best` of the cells `cell` as detection track ids, -1
    for none."""
    best = np.asarray(best).astype(np.int64)
    row = np.asarray(flat.cell_dt_off, dtype=np.int64)[cell] + best
    return _track_ids(np.where(best >= 0, row, -1), flat.dt_id)


def _gt_frame_tables(flat):
    """(frame_off int64[n_gt + 1], the cell and the image id of every
    ground-truth frame): the image at (video, timeline position)."""
    foff = np.asarray(flat.gt_frame_off, dtype=np.int64)
    g_of = np.repeat(np.arange(len(foff) - 1), np.diff(foff))
    cell = np.asarray(flat.gt_cell, dtype=np.int64)[g_of]
    vid = np.asarray(flat.cell_unit, dtype=np.int64)[cell]
    img = np.asarray(flat.tl_image_id)[np.asarray(flat.tl_vid_start, dtype=np.int64)[vid]
                                       + np.asarray(flat.gt_frame_pos, dtype=np.int64)]
    return foff, cell, np.asarray(img)


def _pct(n, d=1.0, width=0):
    """n / d in per cent, "-" without a denominator or for a NaN."""
    text = "{:.2f}".format(100.0 * float(n) / float(d)) if d and n == n else "-"
    return text.rjust(width)


def _windows(ev, vis_rng, vis_lbl):
    """(windows float64[n, 2], their labels): association()'s defaults for None."""
    if vis_rng is None:
        from ..lvis_amodal.eval import Params as LvisParams
        lp = LvisParams(ev.params.iou_type)
        vis_rng = lp.visibility_rng[:5]
        if vis_lbl is None:
            vis_lbl = lp.visibility_rng_lbl[:5]
    rng = np.asarray(vis_rng, dtype=np.float64).reshape(-1, 2)
    if len(rng) > _lib.TRACK_ASSOCIATION_VIS:
        raise ValueError("vis_rng: up to {} visibility windows".format(
            _lib.TRACK_ASSOCIATION_VIS))
    if vis_lbl is None:
        vis_lbl = ["[{:g}, {:g}]".format(lo, hi) for lo, hi in rng.tolist()]
    vis_lbl = [str(x) for x in vis_lbl]
    if len(vis_lbl) != len(rng):
        raise ValueError("vis_lbl: {} labels for {} windows".format(len(vis_lbl), len(rng)))
    return rng, vis_lbl


def association(ev, frame_thr, vis_rng, vis_lbl, per_track, per_frame):
    frame_thr = _frame_thr(ev, frame_thr)
    rng, vis_lbl = _windows(ev, vis_rng, vis_lbl)

    def make():
        from ..._lib import ASSOC_CAT_COLUMNS, ASSOC_TRACK_COLUMNS, ASSOC_VIS_COLUMNS
        t = ev._run.association_table(frame_thr, rng, ev._gt_columns.ann_vis)
        flat = ev._run.flat
        tracks = t["gt_assoc"].astype(np.int64)
        tracks[:, 5] = _track_ids(tracks[:, 5], flat.dt_id)
        # frames: the image at (video, timeline position), the follower's id
        foff, cell, img = _gt_frame_tables(flat)
        return {"columns": {"tracks": list(ASSOC_TRACK_COLUMNS),
                            "cat_counts": list(ASSOC_CAT_COLUMNS),
                            "vis_counts": list(ASSOC_VIS_COLUMNS)},
                "cat_counts": _params_cats(ev, t["cat_counts"], 0),
                "vis_counts": _params_cats(ev, t["vis_counts"], 1),
                "vis_rng": rng.tolist(), "vis_lbl": list(vis_lbl), "frame_thr": frame_thr,
                "tracks": (np.asarray(flat.gt_id), tracks),
                "frames": (foff, img, _follower_ids(flat, cell, t["best"]), t["best_iou"])}
    return _cached(ev._association, (frame_thr, rng.tobytes(), tuple(vis_lbl)), make,
                   (("tracks", per_track), ("frames", per_frame)))


def association_lines(a):
    """TaoEval.association()'s result `a` as a small text table."""
    tot = a["cat_counts"].sum(0)
    w = max([len(x) for x in a["vis_lbl"]] + [10])
    lines = [" track association @[ frame IoU={:0.2f} ]".format(a["frame_thr"]),
             " " + "  ".join("{}={}".format(c, int(v))
                             for c, v in zip(a["columns"]["cat_counts"], tot))
             + "  coverage={}".format(_pct(tot[2], tot[1]))]
    for name, v in zip(a["vis_lbl"], a["vis_counts"].sum(1)):
        lines.append(" " + name.ljust(w) + "{:>11d}".format(int(v[0]))
                     + _pct(v[1], v[0], 9) + _pct(v[2], v[0], 9))
    return lines


def occlusions(ev, frame_thr, vis_rng, recover, len_edges, per_track, per_episode):
    frame_thr = _frame_thr(ev, frame_thr)
    rng = np.asarray(vis_rng, dtype=np.float64).reshape(-1)
    if len(rng) != 2 or not rng[0] <= rng[1]:
        raise ValueError("vis_rng: {} is not one window lo <= hi".format(vis_rng))
    if int(recover) != recover or not 1 <= recover <= _lib.TRACK_OCCLUSION_RECOVER:
        raise ValueError("recover: {} is not an integer in [1, {}]".format(
            recover, _lib.TRACK_OCCLUSION_RECOVER))
    edges = [int(x) for x in np.asarray(len_edges).reshape(-1).tolist()]
    if not 1 <= len(edges) <= _lib.TRACK_OCCLUSION_LEN or edges[0] != 1 \
            or any(a >= b for a, b in zip(edges, edges[1:])) \
            or edges != np.asarray(len_edges).reshape(-1).tolist():
        raise ValueError("len_edges: {} is not 1 to {} ascending integers that start at 1"
                         .format(len_edges, _lib.TRACK_OCCLUSION_LEN))
    key = (frame_thr, float(rng[0]), float(rng[1]), int(recover), tuple(edges))

    def make():
        from ..._lib import (OCC_COUNT_COLUMNS, OCC_EPISODE_COLUMNS, OCC_OUTCOMES,
                             OCC_TRACK_COLUMNS)
        t = ev._run.occlusion_table(frame_thr, key[1:3], key[3], edges, ev._gt_columns.ann_vis)
        flat = ev._run.flat
        gt_id = np.asarray(flat.gt_id)
        foff, cell, img = _gt_frame_tables(flat)
        ep = t["episodes"].astype(np.int64)
        first = foff[ep[:, 0]] + ep[:, 1]
        for col in (4, 5):
            ep[:, col] = _follower_ids(flat, cell[first], ep[:, col])
        lbl = ["{}-{}".format(a, b - 1) if b - 1 > a else str(a)
               for a, b in zip(edges, edges[1:])] + ["{}+".format(edges[-1])]
        return {"columns": {"counts": list(OCC_COUNT_COLUMNS), "tracks": list(OCC_TRACK_COLUMNS),
                            "episodes": list(OCC_EPISODE_COLUMNS),
                            "outcomes": list(OCC_OUTCOMES)},
                "counts": _params_cats(ev, t["counts"], 0), "len_edges": edges, "len_lbl": lbl,
                "vis_rng": [key[1], key[2]], "frame_thr": frame_thr, "recover": key[3],
                "tracks": (gt_id, t["gt_occ"].astype(np.int64)),
                "episodes": (gt_id[ep[:, 0]], img[first], img[first + ep[:, 2] - 1], ep)}
    return _cached(ev._occlusions, key, make,
                   (("tracks", per_track), ("episodes", per_episode)))


def occlusion_lines(e):
    """TaoEval.occlusions()'s result `e` as a small text table, the totals over
    the categories: a line per length bucket."""
    cols = e["columns"]["counts"]
    w = max([len(x) for x in e["len_lbl"]] + [len("length")])
    lines = [" track occlusions @[ frame IoU={:0.2f} | vis=[{:g}, {:g}] | recover={} ]".format(
                 e["frame_thr"], e["vis_rng"][0], e["vis_rng"][1], e["recover"]),
             " " + "length".ljust(w) + "".join(
                 c.rjust(10) for c in ("episodes", "kept%", "switched%", "lost%", "held%"))]
    for name, v in zip(e["len_lbl"], e["counts"].sum(0).tolist()):
        c = dict(zip(cols, v))
        out = c["kept"] + c["switched"] + c["lost"]
        lines.append(" " + name.ljust(w) + "{:>10d}".format(c["episodes"])
                     + "".join(_pct(c[k], out, 10) for k in ("kept", "switched", "lost"))
                     + _pct(c["held"], c["frames"], 10))
    return lines


def identity_ratios(idtp, gt_frames, dt_frames):
    """(IDF1, IDP, IDR) as float64, NaN where the denominator is 0."""
    idtp, gt_frames, dt_frames = (np.asarray(x, dtype=np.float64)
                                  for x in (idtp, gt_frames, dt_frames))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.where(gt_frames + dt_frames > 0, 2 * idtp / (gt_frames + dt_frames), np.nan),
                np.where(dt_frames > 0, idtp / dt_frames, np.nan),
                np.where(gt_frames > 0, idtp / gt_frames, np.nan))


def _identity_numbers(cat_counts):
    """(idf1, idp, idr float64[K], the totals' dict) of the identity's int64[K, 6]."""
    from ..._lib import IDENT_CAT_COLUMNS
    idf1, idp, idr = identity_ratios(cat_counts[:, 4], cat_counts[:, 1], cat_counts[:, 3])
    total = dict(zip(IDENT_CAT_COLUMNS, (int(x) for x in cat_counts.sum(0))))
    total["idfn"] = total["gt_frames"] - total["idtp"]
    total["idfp"] = total["dt_frames"] - total["idtp"]
    for name, v in zip(("idf1", "idp", "idr"),
                       identity_ratios(total["idtp"], total["gt_frames"], total["dt_frames"])):
        total[name] = float(v)
    return idf1, idp, idr, total


def identity(ev, frame_thr, per_track, score_thr=None):
    frame_thr = _frame_thr(ev, frame_thr)
    thr = score_thr_of(ev, score_thr)

    def make():
        from ..._lib import IDENT_CAT_COLUMNS
        t = ev._run.identity_table(frame_thr, _table_thr(ev, thr))
        flat = ev._run.flat
        cat_counts = _params_cats(ev, t["cat_counts"], 0)
        idf1, idp, idr, total = _identity_numbers(cat_counts)
        dt_id, gt_id = (np.asarray(x, dtype=np.int64) for x in (flat.dt_id, flat.gt_id))
        gi, di = t["gt_ident"], t["dt_ident"]
        tracks = np.stack([_track_ids(gi[:, 0], dt_id), gi[:, 1].astype(np.int64),
                           np.diff(np.asarray(flat.gt_frame_off, dtype=np.int64))], axis=1)
        dt_tracks = np.stack([_track_ids(di[:, 0], gt_id), di[:, 1].astype(np.int64),
                              np.diff(np.asarray(flat.dt_frame_off, dtype=np.int64))], axis=1)
        return _with_score_thr(
            {"columns": list(IDENT_CAT_COLUMNS), "cat_counts": cat_counts,
             "idf1": idf1, "idp": idp, "idr": idr, "total": total, "frame_thr": frame_thr,
             "tracks": (gt_id, tracks), "dt_tracks": (dt_id, dt_tracks)}, thr)
    return _cached(ev._identity, _key(thr, frame_thr), make,
                   (("tracks", per_track), ("dt_tracks", per_track)))


HOTA_SCALARS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")


def hota_alphas(alphas):
    """The localisation thresholds as float64: TrackEval's 19 for None, else 1 to
    _lib.TRACK_HOTA_ALPHAS (32) strictly ascending values in (0, 1]."""
    if alphas is None:
        return np.arange(0.05, 0.99, 0.05)
    a = np.asarray(alphas, dtype=np.float64).reshape(-1)
    if not 1 <= len(a) <= _lib.TRACK_HOTA_ALPHAS:
        raise ValueError("alphas: {} values; 1 to {}".format(len(a), _lib.TRACK_HOTA_ALPHAS))
    if not ((a > 0) & (a <= 1)).all():
        raise ValueError("alphas: {} are not all in (0, 1]".format(a.tolist()))
    if (np.diff(a) <= 0).any():
        raise ValueError("alphas: {} do not strictly ascend".format(a.tolist()))
    return a


def hota_ratios(tp, loc, ass, gt_frames, dt_frames):
    """The eight ratios of HOTA's integer tables as float64 in the shape of tp,
    with TrackEval's max(1, .) denominators: tp, loc [.., A] and ass [.., A, 3] in
    fixed point, the frame counts broadcast against tp.  LocA is 1 where tp is 0,
    as in TrackEval."""
    from ..._lib import HOTA_ONE
    tp = np.asarray(tp, dtype=np.int64)
    fn = np.asarray(gt_frames, dtype=np.int64) - tp
    fp = np.asarray(dt_frames, dtype=np.int64) - tp
    tpf, one = tp.astype(np.float64), np.maximum(1, tp).astype(np.float64)
    ass = np.asarray(ass, dtype=np.int64).astype(np.float64) / HOTA_ONE
    loc = np.asarray(loc, dtype=np.int64).astype(np.float64) / HOTA_ONE
    out = {"deta": tpf / np.maximum(1, tp + fn + fp), "detre": tpf / np.maximum(1, tp + fn),
           "detpr": tpf / np.maximum(1, tp + fp), "assa": ass[..., 0] / one,
           "assre": ass[..., 1] / one, "asspr": ass[..., 2] / one,
           "loca": np.where(tp > 0, loc / one, 1.0)}
    out["hota"] = np.sqrt(out["deta"] * out["assa"])
    return out


def hota_scalars(r):
    """The means over alpha of the ratios `r` (last axis) under TrackEval's
    names, and HOTA(0), LocA(0), HOTALocA(0) at the first alpha."""
    out = {name: r[name.lower()].mean(-1) for name in HOTA_SCALARS}
    out["HOTA(0)"], out["LocA(0)"] = r["hota"][..., 0], r["loca"][..., 0]
    out["HOTALocA(0)"] = out["HOTA(0)"] * out["LocA(0)"]
    return out


def _hota_numbers(counts, tp, loc, ass):
    """What hota() forms from the integer tables in the order of params.cat_ids
    (counts int64[K, 4], tp and loc [K, A], ass [K, A, 3]): dict(the HOTA_RATIOS
    float64[K, A], NaN where a category has no frames; "per_cat": the scalars'
    float64[K], masked alike; "total", "mean")."""
    from ..._lib import HOTA_RATIOS
    gt_frames, dt_frames = counts[:, 1:2], counts[:, 3:4]
    r = hota_ratios(tp, loc, ass, gt_frames, dt_frames)
    has = (counts[:, 1] + counts[:, 3]) > 0
    out = {k: np.where(has[:, None], r[k], np.nan) for k in HOTA_RATIOS}
    tot = counts.sum(0)
    total = dict(zip(("gt_tracks", "gt_frames", "dt_tracks", "dt_frames"),
                     (int(x) for x in tot)))
    total.update(tp=tp.sum(0), fn=tot[1] - tp.sum(0), fp=tot[3] - tp.sum(0), loc=loc.sum(0),
                 ass=ass.sum(0))
    rt = hota_ratios(total["tp"], total["loc"], total["ass"], tot[1], tot[3])
    total.update(rt)
    total.update({k: float(v) for k, v in hota_scalars(rt).items()})
    per_cat = hota_scalars(r)
    mean = {k: float(v[has].mean()) if has.any() else float("nan")
            for k, v in per_cat.items()}
    out["per_cat"] = {k: np.where(has, v, np.nan) for k, v in per_cat.items()}
    out["total"], out["mean"] = total, mean
    return out


def hota(ev, alphas, frame_thr, per_frame, score_thr=None):
    frame_thr = _frame_thr(ev, frame_thr)
    alphas = hota_alphas(alphas)
    thr = score_thr_of(ev, score_thr)

    def make():
        t = ev._run.hota_table(alphas - np.finfo(float).eps, frame_thr, _table_thr(ev, thr))
        flat = ev._run.flat
        counts = _params_cats(ev, t["cat_counts"], 0)[:, :4]
        tp, loc, ass = (_params_cats(ev, t[k], 0) for k in ("tp", "loc", "ass"))
        gt_frames, dt_frames = counts[:, 1:2], counts[:, 3:4]
        out = {"alphas": alphas, "frame_thr": frame_thr, "cat_counts": counts, "tp": tp,
               "fn": gt_frames - tp, "fp": dt_frames - tp, "loc": loc, "ass": ass}
        numbers = _hota_numbers(counts, tp, loc, ass)
        del numbers["per_cat"]
        out.update(numbers)
        foff, cell, img = _gt_frame_tables(flat)
        g_of = np.repeat(np.arange(len(foff) - 1), np.diff(foff))
        out["frames"] = (np.asarray(flat.gt_id, dtype=np.int64)[g_of], img,
                         _follower_ids(flat, cell, t["match"]), t["match_iou"])
        return _with_score_thr(out, thr)
    return _cached(ev._hota, _key(thr, alphas.tobytes(), frame_thr), make,
                   (("frames", per_frame),))


def hota_lines(e):
    """TaoEval.hota()'s result `e` as a small text table, in per cent and in
    TrackEval's column order: the detection-averaged total and the class mean."""
    names = list(HOTA_SCALARS) + ["HOTA(0)", "LocA(0)", "HOTALocA(0)"]
    lines = [" track HOTA @[ alphas={:0.2f}:{:0.2f} ({}) | frame IoU={:0.2f}{} ]".format(
                 float(e["alphas"][0]), float(e["alphas"][-1]), len(e["alphas"]), e["frame_thr"],
                 _thr_text(e.get("score_thr"))),
             " " + "".ljust(10) + "".join(n.rjust(12) for n in names)]
    for label, row in (("total", e["total"]), ("class mean", e["mean"])):
        lines.append(" " + label.ljust(10) + "".join(_pct(row[n], width=12) for n in names))
    return lines


CLEAR_SCALARS = ("MOTA", "MOTP", "MODA", "CLR_Re", "CLR_Pr", "MTR", "PTR", "MLR", "sMOTA",
                 "CLR_F1")
CLEAR_INTEGERS = ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag")


def clear_ratios(cat_counts):
    """The ten ratios of clear()'s int64[..., 11] table as float64 in the shape of
    its leading axes, with TrackEval's max(1, .) denominators."""
    from ..._lib import HOTA_ONE
    cc = np.asarray(cat_counts, dtype=np.int64)
    gt_tracks, gt_frames, dt_frames = cc[..., 0], cc[..., 1], cc[..., 3]
    tp, idsw = cc[..., 4], cc[..., 5]
    motp = cc[..., 10].astype(np.float64) / HOTA_ONE
    fn, fp = gt_frames - tp, dt_frames - tp
    g = np.maximum(1, tp + fn).astype(np.float64)
    tr = np.maximum(1, gt_tracks).astype(np.float64)
    return {"mota": (tp - fp - idsw) / g, "motp": motp / np.maximum(1, tp),
            "moda": (tp - fp) / g, "smota": (motp - fp - idsw) / g, "clr_re": tp / g,
            "clr_pr": tp / np.maximum(1, tp + fp).astype(np.float64),
            "clr_f1": tp / np.maximum(1, 2 * tp + fn + fp).astype(np.float64) * 2,
            "mtr": cc[..., 7] / tr, "ptr": cc[..., 8] / tr, "mlr": cc[..., 9] / tr}


def _clear_columns():
    from ..._lib import CLEAR_CAT_COLUMNS, IDENT_CAT_COLUMNS
    return list(IDENT_CAT_COLUMNS[:4]) + list(CLEAR_CAT_COLUMNS)


def _clear_numbers(cc):
    """What clear() forms from its int64[K, 11] table in the order of
    params.cat_ids: dict(the CLEAR_RATIOS float64[K], NaN where a category has no
    frames; "total" without the windows; "mean")."""
    from ..._lib import CLEAR_RATIOS
    r = clear_ratios(cc)
    has = (cc[:, 1] + cc[:, 3]) > 0
    out = {k: np.where(has, r[k], np.nan) for k in CLEAR_RATIOS}
    tot = cc.sum(0)
    total = dict(zip(_clear_columns(), (int(x) for x in tot)))
    total.update(fn=int(tot[1] - tot[4]), fp=int(tot[3] - tot[4]))
    total.update({k: float(v) for k, v in clear_ratios(tot).items()})
    out["total"] = total
    out["mean"] = {k: float(r[k][has].mean()) if has.any() else float("nan")
                   for k in CLEAR_RATIOS}
    return out


def clear(ev, frame_thr, vis_rng, vis_lbl, per_track, per_frame, score_thr=None):
    frame_thr = _frame_thr(ev, frame_thr)
    rng, vis_lbl = _windows(ev, vis_rng, vis_lbl)
    thr = score_thr_of(ev, score_thr)

    def make():
        from ..._lib import CLEAR_VIS_COLUMNS
        t = ev._run.clear_table(frame_thr, rng, ev._gt_columns.ann_vis, _table_thr(ev, thr))
        flat = ev._run.flat
        cc = np.concatenate([_params_cats(ev, t["ident_counts"], 0)[:, :4],
                             _params_cats(ev, t["cat_counts"], 0)], axis=1)
        vis = _params_cats(ev, t["vis_counts"], 1)
        out = {"frame_thr": frame_thr, "cat_counts": cc, "fn": cc[:, 1] - cc[:, 4],
               "fp": cc[:, 3] - cc[:, 4], "vis_counts": vis, "vis_rng": rng.tolist(),
               "vis_lbl": list(vis_lbl),
               "columns": {"cat_counts": _clear_columns(), "vis_counts": list(CLEAR_VIS_COLUMNS),
                           "tracks": ["present", "matched", "idsw", "frag", "tracked"]}}
        out.update(_clear_numbers(cc))
        with np.errstate(divide="ignore", invalid="ignore"):
            out["vis_re"] = np.where(vis[..., 0] > 0, vis[..., 1] / vis[..., 0].astype(np.float64),
                                     np.nan)
        out["total"]["vis_counts"] = vis.sum(1)
        gc = t["gt_clear"].astype(np.int64)
        mt = 5 * gc[:, 1] > 4 * gc[:, 0]
        pt = ~mt & (5 * gc[:, 1] >= gc[:, 0])
        live = (np.asarray(flat.gt_flags)[:len(gc)] & 1) == 0
        tracks = np.stack([gc[:, 0], gc[:, 1], gc[:, 2], np.maximum(gc[:, 3] - 1, 0),
                           np.where(live, 2 * mt + pt, 0)], axis=1)
        out["tracks"] = (np.asarray(flat.gt_id, dtype=np.int64), tracks)
        foff, cell, img = _gt_frame_tables(flat)
        g_of = np.repeat(np.arange(len(foff) - 1), np.diff(foff))
        out["frames"] = (np.asarray(flat.gt_id, dtype=np.int64)[g_of], img,
                         _follower_ids(flat, cell, t["match"]), t["match_iou"], t["sw"])
        return _with_score_thr(out, thr)
    return _cached(ev._clear, _key(thr, frame_thr, rng.tobytes(), tuple(vis_lbl)), make,
                   (("tracks", per_track), ("frames", per_frame)))


def clear_lines(e):
    """TaoEval.clear()'s result `e` as a small text table in TrackEval's CLEAR
    column order: the ratios in per cent and the integers for the total, the
    ratios for the class mean, then CLR_Re and IDSW per visibility window."""
    tot = e["total"]
    ints = {"CLR_TP": tot["tp"], "CLR_FN": tot["fn"], "CLR_FP": tot["fp"], "IDSW": tot["idsw"],
            "MT": tot["mt"], "PT": tot["pt"], "ML": tot["ml"], "Frag": tot["frag"]}
    lines = [" track CLEAR @[ frame IoU={:0.2f}{} ]".format(e["frame_thr"],
                                                           _thr_text(e.get("score_thr"))),
             " " + "".ljust(10) + "".join(n.rjust(9) for n in CLEAR_SCALARS + CLEAR_INTEGERS),
             " " + "total".ljust(10)
             + "".join(_pct(tot[n.lower()], width=9) for n in CLEAR_SCALARS)
             + "".join("{:>9d}".format(int(ints[n])) for n in CLEAR_INTEGERS),
             " " + "class mean".ljust(10)
             + "".join(_pct(e["mean"][n.lower()], width=9) for n in CLEAR_SCALARS)]
    w = max([len(x) for x in e["vis_lbl"]] + [10])
    for name, v in zip(e["vis_lbl"], tot["vis_counts"]):
        lines.append(" " + name.ljust(w) + "{:>11d}".format(int(v[0]))
                     + _pct(v[1], v[0], 9) + "{:>9d}".format(int(v[2])))
    return lines


def identity_lines(e):
    """TaoEval.identity()'s result `e` as a small text table: the totals over
    the categories."""
    t = e["total"]
    return [" track identity @[ frame IoU={:0.2f}{} ]".format(e["frame_thr"],
                                                            _thr_text(e.get("score_thr"))),
            " IDF1={}  IDP={}  IDR={}".format(_pct(t["idf1"]), _pct(t["idp"]), _pct(t["idr"])),
            " " + "  ".join("{}={}".format(c, t[c]) for c in list(e["columns"]) + ["idfn", "idfp"])]


# ---------------------------------------------------------------------------
# tracking_curve(): identity, HOTA and CLEAR over a list of score thresholds
# ---------------------------------------------------------------------------
CURVE_MEASURES = ("identity", "hota", "clear")
CURVE_BEST = (("IDF1", "identity", "idf1"), ("HOTA", "hota", "HOTA"), ("MOTA", "clear", "mota"))
# the per-category [T, K] arrays: (entry, measure)
CURVE_PER_CAT = (("idf1", "identity"), ("hota", "hota"), ("deta", "hota"), ("assa", "hota"),
                 ("mota", "clear"), ("motp", "clear"), ("idsw", "clear"))


def default_score_thrs(dt_score):
    """tracking_curve()'s thresholds for None: the distinct values of the 0 %, 10 %,
    ... 90 % quantiles (method="lower": scores that occur) of the finite scores,
    ascending; [-inf] where no score is finite.  The first is the least finite
    score: every track that is not a NaN (or -inf) passes it."""
    s = np.asarray(dt_score, dtype=np.float64).reshape(-1)
    s = s[np.isfinite(s)]
    if not len(s):
        return np.array([-np.inf])
    return np.unique(np.quantile(s, np.arange(10) / 10.0, method="lower"))


def curve_score_thrs(score_thrs, dt_score):
    """The curve's thresholds as float64[T]: default_score_thrs(dt_score) for None,
    else 1 to _lib.TRACK_SCORE_THRS (64) strictly ascending doubles, none a NaN."""
    if score_thrs is None:
        return default_score_thrs(dt_score)
    a = np.asarray(score_thrs, dtype=np.float64).reshape(-1)
    if not 1 <= len(a) <= _lib.TRACK_SCORE_THRS:
        raise ValueError("score_thrs: {} values; 1 to {}".format(len(a), _lib.TRACK_SCORE_THRS))
    if np.isnan(a).any():
        raise ValueError("score_thrs: {} hold a NaN".format(a.tolist()))
    if (np.diff(a) <= 0).any():
        raise ValueError("score_thrs: {} do not strictly ascend".format(a.tolist()))
    return a


def curve_measures(measures):
    """`measures` as a tuple in the order of CURVE_MEASURES."""
    if isinstance(measures, str):
        measures = (measures,)
    got = [str(m) for m in measures]
    if not got or any(m not in CURVE_MEASURES for m in got) or len(set(got)) != len(got):
        raise ValueError("measures: {} is not a choice of {}".format(
            list(measures), list(CURVE_MEASURES)))
    return tuple(m for m in CURVE_MEASURES if m in got)


def best_index(values):
    """The index of the greatest of `values` that is not a NaN, the FIRST among
    equal maxima (the lowest threshold of an ascending list); -1 if all are NaN
    or there are none."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    ok = ~np.isnan(v)
    if not ok.any():
        return -1
    return int(np.argmax(np.where(ok, v, -np.inf)))      # (argmax: the first of equals)


def best_threshold(values, score_thrs):
    """{"index", "score_thr", "value"} of best_index; index -1 and two NaN for none."""
    i = best_index(values)
    if i < 0:
        return {"index": -1, "score_thr": float("nan"), "value": float("nan")}
    return {"index": i, "score_thr": float(np.asarray(score_thrs)[i]),
            "value": float(np.asarray(values)[i])}


def best_per_category(values, score_thrs):
    """float64[K]: per column of values[T, K] the threshold of best_index, NaN for
    a column of NaNs (a category without frames)."""
    v = np.asarray(values, dtype=np.float64)
    thrs = np.asarray(score_thrs, dtype=np.float64)
    idx = [best_index(v[:, k]) for k in range(v.shape[1])]
    return np.array([thrs[i] if i >= 0 else np.nan for i in idx], dtype=np.float64)


def curve_numbers(score_thrs, cat_counts, tp=None, loc=None, ass=None, clear_counts=None):
    """tracking_curve()'s result from the integer tables in the order of
    params.cat_ids: cat_counts int64[T, K, 6] of the identity, HOTA's tp and loc
    [T, K, A] and ass [T, K, A, 3] and CLEAR's int64[T, K, 7], each None where the
    measure was not asked for.  A row is formed by the functions identity(), hota()
    and clear() form theirs with."""
    T = len(score_thrs)
    out = {"score_thrs": np.asarray(score_thrs, dtype=np.float64),
           "cat_counts": np.asarray(cat_counts, dtype=np.int64)}
    per_cat = {name: [] for name, _ in CURVE_PER_CAT}
    totals, means = [], []
    for t in range(T):
        cc = out["cat_counts"][t]
        idf1, _, _, total = _identity_numbers(cc)
        per_cat["idf1"].append(idf1)
        mean = {}
        if tp is not None:
            h = _hota_numbers(cc[:, :4], tp[t], loc[t], ass[t])
            for name in ("hota", "deta", "assa"):
                per_cat[name].append(h["per_cat"][{"hota": "HOTA", "deta": "DetA",
                                                   "assa": "AssA"}[name]])
            total.update({k: v for k, v in h["total"].items() if isinstance(v, float)})
            mean.update(h["mean"])
        if clear_counts is not None:
            c = _clear_numbers(np.concatenate([cc[:, :4], clear_counts[t]], axis=1))
            per_cat["mota"].append(c["mota"])
            per_cat["motp"].append(c["motp"])
            per_cat["idsw"].append(clear_counts[t][:, 1].astype(np.int64))
            total.update(c["total"])
            mean.update(c["mean"])
        totals.append(total)
        means.append(mean)
    K = out["cat_counts"].shape[1]
    for name, rows in per_cat.items():
        if rows:
            out[name] = np.stack(rows).reshape(T, K)
    out["total"] = {k: np.array([row[k] for row in totals]) for k in totals[0]}
    out["mean"] = {k: np.array([row[k] for row in means]) for k in means[0]}
    out["best"], out["best_per_category"] = {}, {}
    for name, _, key in CURVE_BEST:
        if key in out["total"]:
            out["best"][name] = best_threshold(out["total"][key], out["score_thrs"])
            out["best_per_category"][name] = best_per_category(out[name.lower()],
                                                               out["score_thrs"])
    return out


def tracking_curve(ev, score_thrs, frame_thr, alphas, measures):
    frame_thr = _frame_thr(ev, frame_thr)
    alphas = hota_alphas(alphas)
    measures = curve_measures(measures)
    thrs = curve_score_thrs(score_thrs, ev.flat.dt_score)
    K = len(ev.params.cat_ids)
    tables = _table_thr(ev, np.repeat(thrs[:, None], K, axis=1))
    t = ev._run.curve_tables(frame_thr, tables, alphas - np.finfo(float).eps, measures)
    cats = {k: _params_cats(ev, v, 1) for k, v in t.items()}
    c = curve_numbers(thrs, cats["cat_counts"], cats.get("tp"), cats.get("loc"), cats.get("ass"),
                      cats.get("clear"))
    c.update(frame_thr=frame_thr, alphas=alphas, measures=measures)
    return c


def curve_lines(c):
    """TaoEval.tracking_curve()'s result `c` as a small text table: a line per
    threshold with the totals, "-" for a measure that was not asked for."""
    tot = c["total"]
    names = ("IDF1", "HOTA", "DetA", "AssA", "MOTA")
    keys = ("idf1", "HOTA", "DetA", "AssA", "mota")
    lines = [" tracking curve @[ frame IoU={:0.2f} | {} thresholds ]".format(
                 c["frame_thr"], len(c["score_thrs"])),
             " " + "score>=".rjust(12) + "dt_tracks".rjust(11)
             + "".join(n.rjust(9) for n in names) + "IDSW".rjust(9)]
    for t, thr in enumerate(c["score_thrs"].tolist()):
        lines.append(" " + "{:.6g}".format(thr).rjust(12)
                     + "{:>11d}".format(int(tot["dt_tracks"][t]))
                     + "".join(_pct(tot[k][t], width=9) if k in tot else "-".rjust(9)
                               for k in keys)
                     + ("{:>9d}".format(int(tot["idsw"][t])) if "idsw" in tot
                        else "-".rjust(9)))
    return lines
