"""Plain-Python restatement of the track-level mask IoU of
``TaoEval(iou_type="segm")`` (csrc/track_mask_iou.hip) -- TEST
INFRASTRUCTURE ONLY.  Built on oracle.rle (pycocotools' merge / area /
frPyObjects semantics); the three formulas are written out literally.

A track is a dict {timeline position: mask}, a mask an oracle dict
{"h", "w", "counts"}.  For a shared position t, i_t = area(merge([d_t, g_t],
intersect=True)) and u_t = area(merge([d_t, g_t])) -- both 0 when the frame
sizes differ, because merge then returns an empty mask, and both counted only
up to the pixel at which rleMerge's loop stops: the frame's end, or before it
where both masks finish a run and go on with an empty one, or where the two
current runs have 2^32 pixels left between them (tests/rlepop.py: stop_pixel).
"""
import numpy as np

from oracle import rle


def frame_terms(d, g):
    """(i_t, u_t) of two masks of one frame."""
    return (rle.area(rle.merge([d, g], intersect=True)),
            rle.area(rle.merge([d, g], intersect=False)))


def track_iou(dt, gt, mode, terms=None):
    """IoU of the detection track ``dt`` and the GT track ``gt``.  ``terms``:
    an optional cache {(id(d_t), id(g_t)): (i_t, u_t)} shared by the modes."""
    shared = sorted(set(dt) & set(gt))
    n_union = len(set(dt) | set(gt))

    def it_ut(t):
        if terms is None:
            return frame_terms(dt[t], gt[t])
        key = (id(dt[t]), id(gt[t]))
        if key not in terms:
            terms[key] = frame_terms(dt[t], gt[t])
        return terms[key]

    if mode == "3d_iou":
        inter = sum(it_ut(t)[0] for t in shared)
        union = sum(it_ut(t)[1] for t in shared) \
            + sum(rle.area(m) for t, m in dt.items() if t not in gt) \
            + sum(rle.area(m) for t, m in gt.items() if t not in dt)
        return inter / union if union > 0 else 0.0
    if mode == "avg_iou":
        total = 0.0
        for t in shared:                      # ascending timeline order
            i, u = it_ut(t)
            total += i / u if u > 0 else 0.0
        return total / n_union if n_union else 0.0
    if mode == "imagenetvid":
        hits = 0
        for t in shared:
            i, u = it_ut(t)
            hits += i > 0.5 * u
        return hits / n_union if n_union else 0.0
    raise ValueError(mode)


def shared_frames(dt, gt):
    return len(set(dt) & set(gt))


def tracks_of(frame_off, frame_pos, masks):
    """CSR frame lists + one mask per frame -> list of {position: mask}."""
    off = np.asarray(frame_off, dtype=np.int64)
    pos = np.asarray(frame_pos, dtype=np.int64)
    return [{int(pos[k]): masks[k] for k in range(off[t], off[t + 1])}
            for t in range(len(off) - 1)]


def cell_ious(flat, dt_tracks, gt_tracks, mode, terms=None):
    """IoU vector of the cell tables (iou[cell_iou_off[c] + d*G + g])."""
    d_off = np.asarray(flat.cell_dt_off, dtype=np.int64)
    g_off = np.asarray(flat.cell_gt_off, dtype=np.int64)
    out = []
    for c in range(len(d_off) - 1):
        for d in range(d_off[c], d_off[c + 1]):
            for g in range(g_off[c], g_off[c + 1]):
                out.append(track_iou(dt_tracks[d], gt_tracks[g], mode, terms))
    return np.asarray(out, dtype=np.float64)


def box_polygon(bbox):
    """The polygon the reference gives a prediction without segmentation
    (tao_amodal/results.py:67-68)."""
    x1, y1, w, h = bbox
    x2, y2 = x1 + w, y1 + h
    return [[x1, y1, x1, y2, x2, y2, x2, y1]]


def frame_masks(flat, gt_dataset, preds):
    """The masks of every frame of the track tables: GT frames through
    ann_to_rle of their annotation, prediction frames through their
    segmentation or, without one, their box's polygon."""
    imgs = {im["id"]: im for im in gt_dataset["images"]}
    anns = gt_dataset["annotations"]

    def mask(segm, im):
        return rle.ann_to_rle(segm, im["height"], im["width"])
    gt = [mask(anns[r]["segmentation"], imgs[anns[r]["image_id"]])
          for r in np.asarray(flat.gt_frame_ann).tolist()]
    dt = []
    for r in np.asarray(flat.dt_frame_ann).tolist():
        p = preds[r]
        segm = p["segmentation"] if "segmentation" in p else box_polygon(p["bbox"])
        dt.append(mask(segm, imgs[p["image_id"]]))
    return dt, gt
