"""Score columns outside [0, 1): the populations the score-value tests share
(test_score_values_host.py, test_gpu_score_values.py, the exchange tests), the
expected order, and the small detection sets built around them.

The product takes any double as a score (both JSON readers accept the NaN /
Infinity literals, detectors emit logits).  The reference orders everything
with ``np.argsort(-score, kind="mergesort")``: defined for all of these
values, every NaN last in input order whatever its sign or payload."""
import numpy as np

from tao_amodal_amd.columns import DTColumns, GTColumns
from tao_amodal_amd.synth import synth

KINDS = ("logits", "wide", "specials", "nan")
DBL_MAX = 1.7976931348623157e308
# quiet NaN, the same with the sign bit set, a NaN with a payload
NAN_BITS = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000001],
                    dtype=np.uint64)
NANS = NAN_BITS.view(np.float64)
SPECIALS = np.array([np.inf, -np.inf, -0.0, 0.0, 5e-324, -5e-324, DBL_MAX, -DBL_MAX,
                     -1.0, 0.0])


def _logits(n, rng):
    s = rng.normal(0.0, 4.0, n)
    half = rng.random(n) < 0.5
    s[half] = np.round(s[half], 2)          # exact ties on both sides of zero
    return s


def score_population(kind, n, rng, cat_off=None, nan_cats=None):
    """n scores of one of KINDS.  With `cat_off` (category boundaries of the
    column) the "nan" kind also makes one category all NaN and another all NaN
    but one element: `nan_cats`, or two drawn from those of more than one
    element."""
    if kind == "logits":
        return _logits(n, rng)
    if kind == "wide":
        # subnormals up to near overflow, either sign
        return np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-320, 308, n)
    s = _logits(n, rng)
    if kind == "specials":
        r = rng.random(n)
        for j, v in enumerate(SPECIALS):    # about 5 % each
            s[(r >= 0.05 * j) & (r < 0.05 * (j + 1))] = v
        if n >= 2 * len(SPECIALS):          # (and each at least once)
            s[rng.permutation(n)[:len(SPECIALS)]] = SPECIALS
        return s
    assert kind == "nan", kind
    r = rng.random(n)
    for j, v in enumerate(NANS):            # about 5 % in all
        s[(r >= j / 60.0) & (r < (j + 1) / 60.0)] = v
    if n >= 2 * len(NANS):
        s[rng.permutation(n)[:len(NANS)]] = NANS
    if cat_off is not None:
        many = np.flatnonzero(np.diff(cat_off) > 1)
        if len(many) > 1:
            if nan_cats is None:
                nan_cats = rng.choice(many, 2, replace=False)
            a, b = int(cat_off[nan_cats[0]]), int(cat_off[nan_cats[0] + 1])
            s[a:b] = NANS[rng.integers(0, 3, b - a)]
            a, b = int(cat_off[nan_cats[1]]), int(cat_off[nan_cats[1] + 1])
            one = a + int(rng.integers(0, b - a))
            keep = s[one] if s[one] == s[one] else -2.25
            s[a:b] = NANS[rng.integers(0, 3, b - a)]
            s[one] = keep
    return s


def expected_order(score, cat=None):
    """The reference's order: stable, by category, score descending, NaN last."""
    n = len(score)
    keys = (np.arange(n), -np.asarray(score, dtype=np.float64))
    return np.lexsort(keys if cat is None else keys + (cat,))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_doubles(a, b):
    """Equal bit for bit (NaN payloads and the sign of zero included)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_values(a, b):
    """Equal bit for bit where neither is NaN, NaN in the same places: for
    COMPUTED values (a track's mean), whose NaN carries whatever payload the
    adder that made it chose."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(bits(a)[ok], bits(b)[ok])


# ---------------------------------------------------------------------------
# synthetic sets with a population as their score column
# ---------------------------------------------------------------------------
SYNTH_SETS = {
    # every image over max_dets but the thinned ones: the cut works on these keys
    "cut20": (dict(seed=4, V=4, F=6, C=9, dets_per_frame=50, n_present=4), 20),
    # no cut: NaN everywhere, many small cells
    "cells": (dict(seed=1, V=3, F=8, C=40, dets_per_frame=25), 300),
}


def synth_with_scores(which, kind):
    """(gt, dt, max_dets): a synth() set whose score column is `kind`.  Every
    third image is thinned to 15 detections, so that images at or below
    max_dets exist in both sets; NaN scores go only into those (the order
    Python's sorted() gives a list that holds NaNs depends on the input order:
    the cut of an image over max_dets with NaN scores is no rule to restate)."""
    kw, max_dets = SYNTH_SETS[which]
    gt, dt = synth(**kw)
    rng = np.random.default_rng([kw["seed"], KINDS.index(kind)])
    uniq, inv = np.unique(dt.image_id, return_inverse=True)
    inv = inv.reshape(-1)
    nth = np.zeros(len(dt), np.int64)               # place among its image's detections
    order = np.argsort(inv, kind="stable")
    cnt = np.bincount(inv)
    nth[order] = np.arange(len(dt)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    dt = dt.take(np.flatnonzero((inv % 3 != 0) | (nth < 15)))
    score = score_population(kind, len(dt), rng)
    uniq, inv, cnt = np.unique(dt.image_id, return_inverse=True, return_counts=True)
    over = (cnt > max_dets)[inv.reshape(-1)]
    bad = over & np.isnan(score)
    score[bad] = _logits(int(bad.sum()), rng)
    if kind == "nan":
        assert np.isnan(score).sum() > 5
    dt.score = score
    return gt, dt, max_dets


def _one_category_gt(n_frames, gt_tracks, description):
    """Ground truth JSON: one video, one category; gt_tracks = [(box, frames)]."""
    images = [{"id": 1 + f, "video_id": 1, "frame_index": f, "neg_category_ids": [],
               "not_exhaustive_category_ids": []} for f in range(n_frames)]
    tracks, anns = [], []
    for t, (box, frames) in enumerate(gt_tracks):
        tracks.append({"id": t + 1, "category_id": 1, "video_id": 1})
        for f in frames:
            anns.append({"id": len(anns) + 1, "image_id": 1 + f, "track_id": t + 1,
                         "category_id": 1, "bbox": list(box), "area": box[2] * box[3],
                         "visibility": 1.0, "out_of_frame": False})
    return {"info": {"description": description}, "images": images,
            "videos": [{"id": 1, "name": "v1", "neg_category_ids": [],
                        "not_exhaustive_category_ids": []}],
            "tracks": tracks, "annotations": anns,
            "categories": [{"id": 1, "name": "a", "frequency": "f"}]}


TIE_MAX_DETS = 4
# per image: the scores in file order, and the places (in that list) the cut
# keeps: Python's sorted(reverse=True) is stable, so inside the run of equal
# scores the cut falls in, the FIRST ones in file order stay
TIE_IMAGES = [
    ([-2.5, -2.5, 1.0, -2.5, -2.5, -2.5, -7.0], [0, 1, 2, 3]),          # equal negatives
    ([np.inf, np.inf, -np.inf, np.inf, np.inf, np.inf, 3.0], [0, 1, 3, 4]),
    ([-0.0, 0.0, -1.0, 0.0, -0.0, 5.0, -0.0, 0.0], [0, 1, 3, 5]),       # -0.0 == 0.0
    ([2.0, np.nan, -np.inf], [0, 1, 2]),                                # not cut: NaN allowed
]


def tie_cut_set():
    """(gt, dt, max_dets, kept): a hand-built set whose cut at max_dets falls
    inside a run of equal scores in three images.  The detections of the
    images are interleaved in the file; every detection has a box and a track
    of its own.  kept = sorted file positions of the detections that stay."""
    gtj = _one_category_gt(len(TIE_IMAGES), [([0, 0, 40, 40], range(len(TIE_IMAGES))),
                                             ([100, 0, 40, 40], [0, 2])], "ties at the cut")
    recs = []
    for im, (scores, keep) in enumerate(TIE_IMAGES):
        for j, s in enumerate(scores):
            recs.append((j, im, s, j in keep))
    recs.sort(key=lambda r: (r[0], -r[1]))          # interleaved, images 3 2 1 0
    preds, kept = [], []
    for pos, (j, im, s, keep) in enumerate(recs):
        preds.append({"image_id": 1 + im, "category_id": 1,
                      "bbox": [3 * j, 2 * im, 40 + j, 40 + im], "score": s,
                      "track_id": pos + 1, "video_id": 1})
        if keep:
            kept.append(pos)
    return GTColumns.from_json(gtj), DTColumns.from_json(preds), TIE_MAX_DETS, kept


# ---------------------------------------------------------------------------
# long tracks: the pairwise summation of the track mean
# ---------------------------------------------------------------------------
LONG_FRAMES = 2051
# kept boxes per track: each side of 8 (the running sums), of 128 (the
# recursion), of the 8-aligned split of the halves, the whole video
LONG_COUNTS = [1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 255, 256, 257,
               264, 272, 1000, 2050, 2051]


def long_track_set():
    """(gt, dt): one video, one category, 2051 frames.  Detection tracks with
    LONG_COUNTS boxes (every other one on a random subset of the frames: it
    skips frames), scores alternately from "wide" and from +-1e16 +
    uniform(0, 1), so that any other summation order changes the low bits of
    the mean; two tracks of one score (the second mixes -0.0 and 0.0); one
    track holding +inf and -inf, whose mean is NaN.  File order shuffled."""
    rng = np.random.default_rng(2051)
    gtj = _one_category_gt(LONG_FRAMES, [([0, 10, 50, 50], range(100)),
                                         ([100, 10, 50, 50], range(LONG_FRAMES))],
                           "long tracks")
    frames, scores = [], []
    for t, c in enumerate(LONG_COUNTS):
        fr = np.arange(c) if t % 2 == 0 or c == LONG_FRAMES else \
            np.sort(rng.permutation(LONG_FRAMES)[:c])
        sc = score_population("wide", c, rng) if t % 2 else \
            rng.choice([-1e16, 1e16], c) + rng.random(c)
        frames.append(fr)
        scores.append(sc)
    frames.append(np.arange(300))
    scores.append(np.full(300, -3.75))
    frames.append(np.arange(5, 205))
    scores.append(np.where(rng.random(200) < 0.5, -0.0, 0.0))
    assert len(set(np.signbit(scores[-1]).tolist())) == 2
    frames.append(np.arange(0, 400, 2))
    s = _logits(200, rng)
    s[[3, 150]] = [np.inf, -np.inf]
    scores.append(s)
    img, trk, box, sc = [], [], [], []
    for t, (fr, s) in enumerate(zip(frames, scores)):
        img.append(1 + fr)
        trk.append(np.full(len(fr), t + 1))
        box.append(np.tile([10.0 * t, 10.0, 50.0, 50.0], (len(fr), 1)))
        sc.append(s)
    n = sum(len(x) for x in img)
    dt = DTColumns(image_id=np.concatenate(img).astype(np.int64),
                   category_id=np.ones(n, np.int64), bbox=np.concatenate(box),
                   score=np.concatenate(sc), track_id=np.concatenate(trk).astype(np.int64),
                   video_id=np.ones(n, np.int64))
    return GTColumns.from_json(gtj), dt.take(rng.permutation(n))
