"""Deterministic fixture *inputs* (ground truth + predictions as JSON-shaped
objects).  ``make_golden.py`` runs the reference evaluator on them in the
development container and commits its outputs next to them; the tests then
hold the oracle, the host flatten and the HIP path to those outputs.

F1  random mixed set (5 videos x 20 frames x 6 categories), integer boxes
F2  hand-built quirk set: every tie/boundary/ordering rule of SURVEY.md 8(a)
F3  1203-category sparse set (checks -1 handling and the r/c/f groups)
F4  F1 geometry with arbitrary decimal coordinates (documents the one
    tolerated deviation: frame-sum order of the 3D IoU)
F5  shuffled image ids, colliding track ids, merged categories, >300 dets
    per image
F7  adversarial decimal coordinates: every (detection track, GT track) pair
    has a 3D IoU that is EXACTLY one of the ten IoU thresholds in real
    arithmetic, so its fp64 value lands within a few ulp of the threshold and
    the side it falls on depends on the order the frames are added in -- the
    reference's CPython set order (T/eval.py:83-94) against timeline order
F8  a down-scaled Config 2 with DECIMAL coordinates (16 videos x 300 frames
    x 10 boxes, 100 categories): tracks of hundreds of frames whose per-frame
    terms are inexact in fp64, i.e. the shape real prediction files have.  Its
    golden 3D IoUs are the reference's set-order sums over up to 600 frames
F9  rule-dense cells (rule_cells): the greedy match's tie / ignore / threshold
    / sentinel rules in cells of 2 to 130 GTs, i.e. in every launch route of
    the match (group, single, big) on both levels
F10 scores that are any double (two videos x 6 frames x 3 categories): logits
    on both sides of zero, +-inf, +-0.0, +-5e-324, +-DBL_MAX and NaN (written
    as the NaN / Infinity literals json.dump emits); a track whose mean is
    finite, one whose mean is NaN (+inf and -inf), tracks of one NaN box; a
    category whose best detection scores exactly 0.0 and one whose best scores
    -1.0 (the markers of eval["scores"]).  No image is over 300 detections:
    the order sorted() gives a list that holds NaNs is no rule to restate
F11 prediction-side rules (tests/predrules.py, every motif once): several
    boxes of a track on one image, boxes that vote in the track score and count
    for nothing else, equal track scores ordered by the visiting order of the
    images, track ids 0, 2^31 and 2^40.  Built for max_dets 8 and evaluated by
    the CLI at 300; make_golden_predrules.py records the class API at 3 and 8
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(1, os.path.join(os.path.dirname(__file__), ".."))
from tao_amodal_amd.synth import synth  # noqa: E402


def f1():
    gt, dt = synth(seed=11, V=5, F=20, C=6, dets_per_frame=12,
                   gt_tracks_per_video=6, n_present=3, n_neg=1)
    return gt.to_json(), dt.to_json()


def f3():
    gt, dt = synth(seed=33, V=4, F=6, C=1203, dets_per_frame=20,
                   gt_tracks_per_video=10)
    return gt.to_json(), dt.to_json()


def f4():
    gt, dt = synth(seed=44, V=3, F=12, C=5, dets_per_frame=10,
                   gt_tracks_per_video=6, n_present=3, n_neg=1)
    rng = np.random.default_rng(4)
    gt.ann_bbox = gt.ann_bbox + np.round(rng.random(gt.ann_bbox.shape), 2)
    gt.ann_area = gt.ann_bbox[:, 2] * gt.ann_bbox[:, 3]
    dt.bbox = dt.bbox + np.round(rng.random(dt.bbox.shape), 3)
    return gt.to_json(), dt.to_json()


def f5():
    gt, dt = synth(seed=55, V=3, F=4, C=12, dets_per_frame=340,
                   gt_tracks_per_video=8, n_present=4, n_neg=2,
                   shuffle_image_ids=True, collide_track_ids=True,
                   n_merged=3)
    # quantise scores so that equal scores occur (stable-order paths)
    dt.score = np.round(dt.score, 2)
    return gt.to_json(), dt.to_json()


# --------------------------------------------------------------------------
# F2: hand-built quirks
# --------------------------------------------------------------------------
def f2():
    cats = [
        {"id": 1, "name": "a", "frequency": "f"},
        {"id": 2, "name": "b", "frequency": "c"},
        {"id": 3, "name": "c", "frequency": "r"},
        {"id": 4, "name": "d", "frequency": "f", "merged": [{"id": 5}]},
        {"id": 5, "name": "e", "frequency": "c"},
        {"id": 6, "name": "f", "frequency": "r"},
        {"id": 7, "name": "g", "frequency": "c"},
        {"id": 9, "name": "h", "frequency": "f"},
    ]
    videos = [
        {"id": 10, "name": "v10", "neg_category_ids": [3],
         "not_exhaustive_category_ids": [2]},
        {"id": 20, "name": "v20", "neg_category_ids": [6],
         "not_exhaustive_category_ids": []},
        {"id": 30, "name": "v30", "neg_category_ids": [],
         "not_exhaustive_category_ids": []},
    ]
    # image ids deliberately out of order (CPython set-iteration order leak,
    # SURVEY 8(a) a10) -- 12 frames for v10, 11 for v20, 3 for v30
    v10_imgs = [1000003, 5, 999999999, 12, 70000, 8, 33, 64, 65, 1024, 4097, 7]
    v20_imgs = [200 + 7 * k for k in range(11)]
    v30_imgs = [3001, 3000, 3002]
    images = []
    for vid, ids in ((10, v10_imgs), (20, v20_imgs), (30, v30_imgs)):
        v = [x for x in videos if x["id"] == vid][0]
        for f, i in enumerate(ids):
            images.append({
                "id": i, "video_id": vid, "frame_index": 30 * f,
                "neg_category_ids": list(v["neg_category_ids"]),
                "not_exhaustive_category_ids":
                    list(v["not_exhaustive_category_ids"])})
    # image-level lists may differ from the video-level ones
    images[3]["neg_category_ids"] = [3, 7]
    images[4]["not_exhaustive_category_ids"] = []

    tracks, anns = [], []

    def add_gt(tid, cat, vid, frames_boxes, vis=1.0, oof=False, ignore=None,
               trk_ignore=False, area=None, first_ann_id=None):
        t = {"id": tid, "category_id": cat, "video_id": vid}
        if trk_ignore:
            t["ignore"] = 1
        tracks.append(t)
        for k, (img, box) in enumerate(frames_boxes):
            a = {"id": (first_ann_id + k) if first_ann_id is not None
                 else len(anns) + 1,
                 "image_id": img, "track_id": tid, "category_id": cat,
                 "bbox": list(box),
                 "area": box[2] * box[3] if area is None else area[k],
                 "visibility": vis[k] if isinstance(vis, list) else vis,
                 "out_of_frame": oof[k] if isinstance(oof, list) else oof}
            if ignore is not None and ignore[k]:
                a["ignore"] = 1
            anns.append(a)

    # ---- video 10 -------------------------------------------------------
    box_a = [100, 100, 50, 50]
    # 101 and 102: identical boxes on every frame -> IoU tie (later GT wins)
    vis12 = [0.0, 0.05, 0.1, 0.1, 0.3, 0.8, 0.8, 0.9, 1.0, 1.0, 0.79, 0.81]
    add_gt(101, 1, 10, [(i, box_a) for i in v10_imgs], vis=vis12)
    add_gt(102, 1, 10, [(i, box_a) for i in v10_imgs], vis=vis12[::-1])
    # 103: duration exactly 3 (short AND medium), mean area exactly 1024
    add_gt(103, 2, 10, [(i, [300, 50, 32, 32]) for i in v10_imgs[:3]],
           vis=[0.8, 0.1, 1.0])
    # 104: duration exactly 10 (medium AND long), mean area exactly 9216
    add_gt(104, 2, 10, [(i, [400, 200, 96, 96]) for i in v10_imgs[:10]],
           vis=0.5)
    # 105: category 5 is merged into 4
    add_gt(105, 5, 10, [(i, [600, 300, 40, 60]) for i in v10_imgs[2:9]],
           vis=0.9, oof=[False, True, True, False, False, True, False])
    # 106: track-level ignore + some annotation-level ignore flags
    add_gt(106, 1, 10, [(i, [700, 100, 80, 80]) for i in v10_imgs[:6]],
           vis=1.0, ignore=[1, 0, 1, 0, 0, 1], trk_ignore=True)
    # 107: exactly 5 frames with visibility < 0.8 -> ignored by the HP range
    add_gt(107, 7, 10, [(i, [50, 400, 64, 64]) for i in v10_imgs[:8]],
           vis=[0.1, 0.2, 0.3, 0.4, 0.5, 0.8, 0.9, 1.0])
    # 108: exactly 6 such frames -> evaluated by the HP range
    add_gt(108, 7, 10, [(i, [250, 400, 64, 64]) for i in v10_imgs[:8]],
           vis=[0.1, 0.2, 0.3, 0.4, 0.5, 0.79, 0.9, 1.0])
    # 109: one zero-area annotation (dropped by the strict area>0 filter),
    #      negative / partly out-of-frame coordinates
    add_gt(109, 1, 10, [(v10_imgs[0], [-20, -10, 60, 40]),
                        (v10_imgs[1], [-20, -10, 0, 40]),
                        (v10_imgs[2], [1250, 700, 60, 40]),
                        (v10_imgs[3], [-20, -10, 60, 40])],
           vis=0.3, oof=True)
    # ---- video 20 -------------------------------------------------------
    add_gt(201, 1, 20, [(i, [10 + 5 * k, 20, 30, 30])
                        for k, i in enumerate(v20_imgs)], vis=0.95)
    add_gt(202, 2, 20, [(i, [500, 20 + 3 * k, 200, 100])
                        for k, i in enumerate(v20_imgs[:4])], vis=0.05,
           oof=True)
    add_gt(203, 3, 20, [(i, [900, 500, 20, 20]) for i in v20_imgs[5:7]],
           vis=0.6)
    # category 9: ground truth but never predicted (precision 0, recall 0)
    add_gt(204, 9, 20, [(i, [40, 600, 100, 100]) for i in v20_imgs[:5]],
           vis=1.0)
    # ---- video 30: id sentinels ----------------------------------------
    # annotation id 0 (LVIS "unmatched" sentinel) and track id -1 (TAO one)
    add_gt(-1, 1, 30, [(i, [100, 100, 100, 100]) for i in v30_imgs],
           vis=1.0, first_ann_id=0)
    add_gt(301, 1, 30, [(i, [400, 100, 100, 100]) for i in v30_imgs],
           vis=0.5, first_ann_id=9001)

    preds = []

    def add_dt(tid, cat, vid, frames_boxes, score):
        for k, (img, box) in enumerate(frames_boxes):
            preds.append({"image_id": img, "category_id": cat,
                          "bbox": list(box),
                          "score": score[k] if isinstance(score, list)
                          else score,
                          "track_id": tid, "video_id": vid})

    # exact copy of the tied GT pair
    add_dt(1, 1, 10, [(i, box_a) for i in v10_imgs], 0.9)
    # second detection on the pair with a smaller IoU, equal score to a third
    add_dt(2, 1, 10, [(i, [104, 104, 50, 50]) for i in v10_imgs], 0.8)
    add_dt(3, 1, 10, [(i, [96, 98, 52, 50]) for i in v10_imgs], 0.8)
    # matches only the ignored track 106
    add_dt(4, 1, 10, [(i, [702, 101, 80, 80]) for i in v10_imgs[:6]], 0.7)
    # not-exhaustive category 2: an unmatched one (ignored) and matches
    add_dt(5, 2, 10, [(i, [1000, 600, 30, 30]) for i in v10_imgs[:4]], 0.6)
    add_dt(6, 2, 10, [(i, [301, 51, 32, 32]) for i in v10_imgs[:3]],
           [0.5, 0.7, 0.9])                      # non-uniform scores -> mean
    add_dt(7, 2, 10, [(i, [398, 203, 99, 94]) for i in v10_imgs[:10]], 0.55)
    # negative category 3: plain false positives
    add_dt(8, 3, 10, [(i, [10, 10, 20, 20]) for i in v10_imgs[:5]], 0.95)
    # merged category: predicted as 5, scored as 4
    add_dt(9, 5, 10, [(i, [601, 301, 40, 60]) for i in v10_imgs[2:9]], 0.85)
    # category 7: HP tracks
    add_dt(10, 7, 10, [(i, [52, 402, 64, 64]) for i in v10_imgs[:8]], 0.75)
    add_dt(11, 7, 10, [(i, [251, 399, 64, 64]) for i in v10_imgs[:8]], 0.65)
    # category 6 in video 10: neither present nor negative -> dropped
    add_dt(12, 6, 10, [(i, [5, 5, 50, 50]) for i in v10_imgs[:3]], 0.99)
    # category 42 does not exist in the ground truth -> dropped
    add_dt(13, 42, 10, [(i, [5, 5, 50, 50]) for i in v10_imgs[:2]], 0.98)
    # zero-width detection (dropped) inside an otherwise valid track,
    # negative coordinates
    add_dt(14, 1, 10, [(v10_imgs[0], [-18, -12, 60, 40]),
                       (v10_imgs[1], [-18, -12, 0, 40]),
                       (v10_imgs[2], [1248, 698, 60, 40]),
                       (v10_imgs[3], [-20, -10, 60, 40])], 0.45)
    # track id 7 / 1 re-used in video 20 (make_track_ids_unique)
    add_dt(7, 1, 20, [(i, [12 + 5 * k, 21, 30, 30])
                      for k, i in enumerate(v20_imgs)], 0.9)
    add_dt(1, 2, 20, [(i, [480, 25 + 3 * k, 210, 100])
                      for k, i in enumerate(v20_imgs[:4])], 0.4)
    add_dt(20, 6, 20, [(i, [100, 100, 10, 10]) for i in v20_imgs[:2]], 0.3)
    add_dt(21, 3, 20, [(i, [901, 501, 20, 20]) for i in v20_imgs[4:8]], 0.35)
    # category 7 is unlisted in video 20 -> dropped
    add_dt(22, 7, 20, [(i, [300, 300, 64, 64]) for i in v20_imgs[:3]], 0.97)
    # more than 300 detections in one image (top-300 cut, equal scores)
    big = v20_imgs[9]
    for k in range(330):
        add_dt(1000 + k, 1 if k % 3 else 6, 20,
               [(big, [(k * 37) % 1200, (k * 91) % 650, 20 + k % 50,
                       20 + (k * 7) % 60])],
               round(0.05 + (k % 40) * 0.02, 2))
    # video 30: detection track id 0 (never consumes its GT) + two others
    add_dt(0, 1, 30, [(i, [100, 100, 100, 100]) for i in v30_imgs], 0.9)
    add_dt(31, 1, 30, [(i, [102, 100, 100, 100]) for i in v30_imgs], 0.8)
    add_dt(32, 1, 30, [(i, [398, 101, 100, 100]) for i in v30_imgs], 0.7)
    add_dt(33, 1, 30, [(i, [403, 100, 100, 100]) for i in v30_imgs], 0.6)

    gt = {"info": {"description": "quirks"}, "images": images,
          "videos": videos, "tracks": tracks, "annotations": anns,
          "categories": cats}
    return gt, preds


def f7():
    rng = np.random.default_rng(77)
    cats = [{"id": c, "name": "c%d" % c, "frequency": "rcf"[c % 3]}
            for c in (1, 2, 3)]
    videos, images, tracks, anns, preds = [], [], [], [], []
    thr = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]
    next_img, next_trk, next_dt = 1, 1, 1
    for v in range(1, 5):
        videos.append({"id": v, "name": "v%d" % v, "neg_category_ids": [],
                       "not_exhaustive_category_ids": []})
        n_fr = 8 + 3 * v
        # ids spread so that the sets' slot order is not the timeline order
        ids = (next_img + rng.permutation(n_fr * 37)[:n_fr]).tolist()
        next_img += n_fr * 37
        for f, i in enumerate(ids):
            images.append({"id": int(i), "video_id": v, "frame_index": 30 * f,
                           "neg_category_ids": [],
                           "not_exhaustive_category_ids": []})
        for g in range(6):
            cat = 1 + g % 3
            lo = int(rng.integers(0, n_fr - 5))
            hi = int(rng.integers(lo + 5, n_fr + 1))
            x = rng.integers(0, 900, hi - lo) + rng.integers(0, 100, hi - lo) / 100
            y = rng.integers(0, 500, hi - lo) + rng.integers(0, 100, hi - lo) / 100
            w = rng.integers(20, 300, hi - lo) + rng.integers(0, 10, hi - lo) / 10
            # heights are multiples of 0.2: h * t has at most two decimals
            h = rng.integers(100, 1000, hi - lo) / 5.0
            tracks.append({"id": next_trk, "category_id": cat, "video_id": v})
            for k in range(hi - lo):
                box = [float(x[k]), float(y[k]), float(w[k]), float(h[k])]
                anns.append({"id": len(anns) + 1, "image_id": int(ids[lo + k]),
                             "track_id": next_trk, "category_id": cat,
                             "bbox": box, "area": box[2] * box[3],
                             "visibility": 1.0, "out_of_frame": False})
            # detection tracks covering exactly the same frames, the same
            # boxes with the height scaled by a threshold: IoU = t per frame
            for t in rng.permutation(thr)[:5]:
                score = float(rng.integers(1, 1000)) / 1000
                for k in range(hi - lo):
                    hh = float(np.round(h[k] * t, 2))
                    preds.append({"image_id": int(ids[lo + k]),
                                  "category_id": cat,
                                  "bbox": [float(x[k]), float(y[k]), float(w[k]), hh],
                                  "score": score, "track_id": next_dt,
                                  "video_id": v})
                next_dt += 1
            next_trk += 1
    gt = {"info": {"description": "threshold-straddling 3D IoUs"},
          "images": images, "videos": videos, "tracks": tracks,
          "annotations": anns, "categories": cats}
    return gt, preds


def f8():
    gt, dt = synth(seed=88, V=16, F=300, C=100, dets_per_frame=10,
                   decimal=True, shuffle_image_ids=True)
    return gt.to_json(), dt.to_json()


# --------------------------------------------------------------------------
# rule-dense cells of any size (F9, tests/test_gpu_match_routes.py)
# --------------------------------------------------------------------------
# A motif is a few GT and detection tracks of category 1 in a slot of
# 128 x 112 pixels no other box reaches, so the image-level cells (frame,
# category) and the track-level cell (video, category) hold the same rules.
# Integer boxes: every IoU is a quotient of integers.  Most motifs live on
# frames 0 and 1, the ones where a detection has two candidate GTs on frame 0
# only: frame 1's cell takes the group kernel's closed form, frame 0's its
# sequential greedy.
T2, T3, F0 = [0, 1], [0, 1, 2], [0]
SLOT_W, SLOT_H, PAD_Y, PAD_PITCH, PAD_PER_ROW = 128, 112, 360, 12, 85


def _m_tie_vis(add):
    # identical GTs; visibility 0.5 is regular in range [0.1, 0.8] and ignored
    # in [0.8, 1], 0.9 the other way round: the tie spans the ignore order
    add.gt([0, 0, 50, 50], F0, vis=0.5)
    add.gt([0, 0, 50, 50], F0, vis=0.9)
    add.dt([0, 0, 50, 50], F0, 0.9)
    add.dt([4, 4, 50, 50], F0, 0.8)


def _m_tie_ignored(first):
    def motif(add):
        # an ignored and a regular GT with one box, the ignored one first or second
        add.gt([0, 0, 50, 50], F0, ignore=first)
        add.gt([0, 0, 50, 50], F0, ignore=not first)
        add.dt([0, 0, 50, 50], F0, 0.7)
        add.dt([2, 0, 50, 50], F0, 0.6)
    return motif


def _m_ignored_best(add):
    # IoU 1 with an ignored GT, 0.8 with a regular one
    add.gt([0, 0, 20, 20], F0, ignore=True)
    add.gt([0, 0, 20, 16], F0)
    add.dt([0, 0, 20, 20], F0, 0.85)


def _m_thresholds(ks):
    def motif(add):
        # [x, y, k, 1] against [x, y, 20, 1]: IoU exactly k / 20, on every
        # default threshold (np.linspace: 0.9 meets 0.8999999999999999)
        for j, k in enumerate(ks):
            add.gt([0, 4 * j, 20, 1], T2)
            add.dt([0, 4 * j, k, 1], T2, 0.5 + 0.01 * j)
    return motif


def _m_iou_one(add):
    # reaches the 1 - 1e-10 clamp of the top threshold
    add.gt([0, 0, 30, 20], T2)
    add.dt([0, 0, 30, 20], T2, 0.55)


def _m_vis_bounds(add):
    # visibility exactly on the image level's range bounds, out of frame
    for x, kw in ((0, {"vis": 0.1}), (24, {"vis": 0.8}), (48, {"vis": 0.0}),
                  (72, {"oof": True})):
        add.gt([x, 0, 20, 20], T2, **kw)
        add.dt([x, 0, 20, 20], T2, 0.65)


def _m_area_bounds(add):
    # mean areas exactly 1024 and 9216 (track level)
    add.gt([0, 0, 32, 32], T2)
    add.gt([32, 0, 96, 96], T2)
    add.dt([0, 0, 32, 32], T2, 0.75)
    add.dt([31, 1, 96, 96], T2, 0.75)


def _m_duration_bounds(add):
    # durations exactly 3 and 10 (track level)
    for x, fr in ((0, T3), (24, list(range(10)))):
        add.gt([x, 0, 20, 20], fr)
        add.dt([x, 0, 20, 20], fr, 0.6)


def _m_hp_bounds(add):
    # exactly 5 (the HP range ignores the track) and 6 frames below 0.8
    for x, last in ((0, 0.8), (24, 0.2)):
        add.gt([x, 0, 20, 20], list(range(6)), vis=[0.1, 0.5, 0.79, 0.3, 0.0, last])
        add.dt([x + 1, 0, 20, 20], list(range(6)), 0.45)


def _m_flags(add):
    # annotation ignore only, track ignore only, a zero-area annotation
    add.gt([0, 0, 20, 20], T2, ann_ignore=True)
    add.gt([24, 0, 20, 20], T2, trk_ignore=True)
    add.gt([48, 0, 20, 20], T2, zero_at=1)
    for x in (0, 24, 48):
        add.dt([x, 0, 20, 20], T2, 0.5)


def _m_equal_scores(add):
    # equal scores: the earlier detection takes the GT
    add.gt([0, 0, 40, 20], T2)
    add.dt([0, 0, 40, 20], T2, 0.4)
    add.dt([0, 0, 40, 20], T2, 0.4)


def _m_no_consume(add):
    # a detection track id <= 0 does not consume its GT (track level)
    add.gt([0, 0, 40, 20], T2)
    add.dt([0, 0, 40, 20], T2, 0.95, no_consume=True)
    add.dt([1, 0, 40, 20], T2, 0.35)


def _m_hidden(add):
    # once per file: GT annotation id 0 (image level) on GT track id -1
    add.gt([0, 0, 40, 40], T2, hidden=True)
    add.gt([48, 0, 40, 40], T2)
    for box, score in (([0, 0], 0.8), ([2, 0], 0.7), ([47, 1], 0.6), ([52, 0], 0.5)):
        add.dt(box + [40, 40], T2, score, no_consume=score == 0.8)


# (GT tracks, builder, frames of the video it needs)
RULE_MOTIFS = [
    (2, _m_tie_vis, 2), (5, _m_thresholds(range(10, 15)), 2), (1, _m_equal_scores, 2),
    (2, _m_tie_ignored(True), 1), (4, _m_vis_bounds, 2), (1, _m_no_consume, 2),
    (2, _m_ignored_best, 1), (5, _m_thresholds(range(15, 20)), 2), (1, _m_iou_one, 2),
    (2, _m_tie_ignored(False), 1), (2, _m_area_bounds, 2), (2, _m_duration_bounds, 10),
    (2, _m_hp_bounds, 6), (3, _m_flags, 2),
]


def rule_cells(sizes, hidden_in=0, negative_ids=True):
    """(gt, predictions) JSON objects: one video of category 1 per entry of
    `sizes`, whose track-level cell holds sizes[i] GT tracks and whose frame-0
    image cell sizes[i] GTs.  Video i takes the motifs in turn from motif i on,
    each that still fits, and is padded with one-frame GTs and two detections
    that overlap nothing.  Video `hidden_in` also holds the id sentinels.
    Non-consuming detections get track ids 0, -1, -2, ... -- only the first
    one when `negative_ids` is False (the device flatten takes none below 0)."""
    images, videos, tracks, anns, preds = [], [], [], [], []
    n = {"img": 0, "trk": 0, "ann": 0, "dtrk": 0, "nc": 0}

    class Add:
        def __init__(self, vid, ox, oy):
            self.vid, self.ox, self.oy = vid, ox, oy

        def box(self, b):
            return [b[0] + self.ox, b[1] + self.oy, b[2], b[3]]

        def gt(self, box, frames, vis=1.0, oof=False, ignore=False,
               ann_ignore=False, trk_ignore=False, zero_at=None, hidden=False):
            n["trk"] += 0 if hidden else 1
            tid = -1 if hidden else n["trk"]
            tracks.append({"id": tid, "category_id": 1, "video_id": self.vid})
            if ignore or trk_ignore:
                tracks[-1]["ignore"] = 1
            for k, fr in enumerate(frames):
                b = self.box(box)
                b[2] = 0 if zero_at == k else b[2]
                n["ann"] += 0 if hidden and k == 0 else 1
                anns.append({"id": 0 if hidden and k == 0 else n["ann"],
                             "image_id": img0 + fr, "track_id": tid,
                             "category_id": 1, "bbox": b, "area": b[2] * b[3],
                             "visibility": vis[k] if isinstance(vis, list) else vis,
                             "out_of_frame": oof})
                if ignore or ann_ignore:
                    anns[-1]["ignore"] = 1

        def dt(self, box, frames, score, no_consume=False):
            if no_consume and (negative_ids or n["nc"] == 0):
                tid = -n["nc"]       # unique: make_track_ids_unique keeps it
                n["nc"] += 1
            else:
                n["dtrk"] += 1
                tid = n["dtrk"]
            for fr in frames:
                preds.append({"image_id": img0 + fr, "category_id": 1,
                              "bbox": self.box(box), "score": score,
                              "track_id": tid, "video_id": self.vid})

    for i, G in enumerate(sizes):
        vid = i + 1
        chosen = [(2, _m_hidden, 2)] if i == hidden_in else []
        for j in range(len(RULE_MOTIFS)):
            m = RULE_MOTIFS[(i + j) % len(RULE_MOTIFS)]
            if sum(c[0] for c in chosen) + m[0] <= G:
                chosen.append(m)
        n_pad = G - sum(c[0] for c in chosen)
        if len(chosen) > 8 * (PAD_Y // SLOT_H) or n_pad > PAD_PER_ROW * 50:
            raise ValueError("cell too large for one image")
        videos.append({"id": vid, "name": "v%d" % vid, "neg_category_ids": [],
                       "not_exhaustive_category_ids": []})
        img0 = n["img"] + 1
        for fr in range(max(c[2] for c in chosen) if chosen else 1):
            n["img"] += 1
            images.append({"id": n["img"], "video_id": vid, "frame_index": fr,
                           "neg_category_ids": [], "not_exhaustive_category_ids": []})
        for s, (_, fn, _) in enumerate(chosen):
            fn(Add(vid, (s % 8) * SLOT_W, (s // 8) * SLOT_H))
        pad = Add(vid, 0, PAD_Y)
        for p in range(n_pad):
            pad.gt([(p % PAD_PER_ROW) * PAD_PITCH, (p // PAD_PER_ROW) * PAD_PITCH, 8, 8], [0])
        for p in range(2):
            pad.dt([p * PAD_PITCH, 620, 8, 8], [0], 0.3 + 0.1 * p)
    gt = {"info": {"description": "rule-dense cells"}, "images": images,
          "videos": videos, "tracks": tracks, "annotations": anns,
          "categories": [{"id": 1, "name": "a", "frequency": "f"}]}
    return gt, preds


# F9: runs of group-sized cells (<= 8 GTs), a cell of 64 GTs
# (match_kernel), 65 / 96 / 97 / 130 GTs (match_big_kernel, either side of the
# 64-GT and the 32-bit word bounds), both levels
F9_SIZES = [8, 6, 8, 5, 7, 8, 64, 65, 96, 97, 130]


def f9():
    return rule_cells(F9_SIZES, hidden_in=6, negative_ids=False)


# --------------------------------------------------------------------------
# F10: scores that are any double
# --------------------------------------------------------------------------
DBL_MAX = 1.7976931348623157e308


def f10():
    inf, nan = float("inf"), float("nan")
    cats = [{"id": c, "name": "c%d" % c, "frequency": "fcr"[c - 1]} for c in (1, 2, 3)]
    videos, images, tracks, anns, preds = [], [], [], [], []
    for v in (1, 2):
        videos.append({"id": v, "name": "v%d" % v, "neg_category_ids": [],
                       "not_exhaustive_category_ids": []})
        for f in range(6):
            images.append({"id": 10 * v + f, "video_id": v, "frame_index": 30 * f,
                           "neg_category_ids": [], "not_exhaustive_category_ids": []})
        for c in (1, 2, 3):
            # two GT tracks per (video, category): recall moves in steps
            for g in range(2):
                tid = 100 * v + 10 * c + g
                tracks.append({"id": tid, "category_id": c, "video_id": v})
                for f in range(6 - 2 * g):
                    box = [200 * c + 400 * g, 50 + 5 * f, 60, 60]
                    anns.append({"id": len(anns) + 1, "image_id": 10 * v + f,
                                 "track_id": tid, "category_id": c, "bbox": box,
                                 "area": box[2] * box[3], "visibility": 1.0,
                                 "out_of_frame": False})
    n_trk = [0]

    def add_dt(v, c, frames, score, dx=0, g=0):
        n_trk[0] += 1
        for k, f in enumerate(frames):
            preds.append({"image_id": 10 * v + f, "category_id": c,
                          "bbox": [200 * c + 400 * g + dx, 50 + 5 * f, 60, 60],
                          "score": score[k] if isinstance(score, list) else score,
                          "track_id": n_trk[0], "video_id": v})

    six = list(range(6))
    # category 1: a track with differing scores (mean), one with +inf and -inf
    # (mean NaN: last at the track level), one of a single NaN box
    add_dt(1, 1, six, [2.5, -1.25, 0.5, 5e-324, -0.0, DBL_MAX])
    add_dt(1, 1, six, [inf, -inf, 1.0, inf, -3.0, 0.0], dx=4)
    add_dt(1, 1, [2], nan, dx=8)
    add_dt(1, 1, six[:4], -DBL_MAX, g=1)
    add_dt(2, 1, six, inf)
    add_dt(2, 1, six, -1.25, dx=6)
    add_dt(2, 1, [4], nan, dx=2)
    add_dt(2, 1, six[:4], 2.5, g=1)
    # category 2: the best detection has score exactly 0.0 (-0.0 ties with it,
    # in file order), the rest lies below zero down to -inf
    add_dt(1, 2, six, 0.0)
    add_dt(1, 2, six, -0.0, dx=3)
    add_dt(1, 2, six[:4], -5e-324, g=1)
    add_dt(1, 2, six, -inf, dx=40)
    add_dt(2, 2, six, -0.0, dx=1)
    add_dt(2, 2, six[:4], 0.0, g=1)
    add_dt(2, 2, six, -2.0, dx=5)
    add_dt(2, 2, [0], nan, dx=9)
    # category 3: the best detection has score exactly -1.0
    add_dt(1, 3, six, -1.0)
    add_dt(1, 3, six[:4], -1.5, g=1)
    add_dt(1, 3, six, -DBL_MAX, dx=7)
    add_dt(2, 3, six, -1.0, dx=2)
    add_dt(2, 3, six[:4], -1.0, g=1)
    add_dt(2, 3, six, [-1.0, -2.0, -1.0, -inf, -1.0, -1.0], dx=30)
    add_dt(2, 3, [5], nan, dx=1)
    gt = {"info": {"description": "scores that are any double"}, "images": images,
          "videos": videos, "tracks": tracks, "annotations": anns, "categories": cats}
    return gt, preds


def f11():
    import predrules
    s = predrules.sized(max_dets=8, wide=True)
    return s.gt, s.preds


ALL = {"f1": f1, "f2": f2, "f3": f3, "f4": f4, "f5": f5, "f7": f7, "f8": f8,
       "f9": f9, "f10": f10, "f11": f11}
# big fixtures: inputs stored gzipped, image level reduced to the integer
# match counts + precision / recall + results + text (make_golden.py)
LITE = {"f8"}
