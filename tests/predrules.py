"""Rule-dense PREDICTION sets: the prediction-side rules of the table build
(TaoResults / LVISResults, limit_dets_per_image, get_ann_ids,
group_ann_tracks, the per-track dict of compute_iou) as small motifs, shared by
tests/golden/fixtures.py (F11), tests/golden/make_golden_predrules.py,
test_pred_rules_host.py and test_gpu_pred_rules.py.

The ground truth is the module's own and fixed (ground_truth: five videos, not
one taken from synth() or a fixture): one motif lives in one video of 12
frames, so that under ``max_dets`` 3 no image outside the ``cut`` motif is
over-full -- the motifs packed into fewer videos would cut each other's boxes
-- and every motif knows the tracks, categories and negative lists it plays
against.  What a motif names is then what the set holds
(test_pred_rules_host.py::test_sets_hold_what_they_name).  Boxes
are integers (one box of w * h == inf aside, which no IoU meets).

  ties       five tracks of score exactly 0.5 and one whose boxes score 0.25
             and 0.75, in one (video, category) cell; their first boxes lie on
             different images, visited in CPython set order
  dup_frame  tracks with 2 and 3 boxes on one image (first, middle, last frame;
             one track of duplicates only); 3 frames / len 4, 10 frames / len 11
  votes      zero-width, zero-height, w * h == inf and negative-area boxes
             among valid ones, a track of such boxes only, an unknown and a
             merged-away category
  cut        images with max_dets, max_dets + 1 and max_dets + 2 boxes; a zero
             area and an unknown-category box displace a valid one; a track
             that loses its first box, one that loses every box, equal scores
             at the cut
  ids        track id 0, optionally ids at 2^31 and 2^40, predictions in
             categories without ground truth in the video (listed as negative:
             kept, unlisted: dropped)

``clash_inputs`` derives the inputs the reference rejects (and the one it does
not) from a set.  ``sized`` pads a set with one-box filler tracks on fresh
images to an exact number of boxes / tracks / images."""
import copy

import numpy as np

from tao_amodal_amd.columns import DTColumns, GTColumns

MOTIFS = ("ties", "dup_frame", "votes", "cut", "ids")
# F2's out-of-order image ids (the large one shortened: eight times it stays
# below 2^31), times 8 plus the video's number
BASE_IDS = [1000003, 5, 99999999, 12, 70000, 8, 33, 64, 65, 1024, 4097, 7]
FILL_VIDEO, FILL_IMG0 = 60, 3000001
G1, G2A, G2B = [100, 100, 50, 50], [300, 50, 32, 32], [400, 200, 96, 96]
G4, G7 = [600, 300, 40, 60], [50, 400, 64, 64]
TIE_FRAMES = [3, 0, 4, 1, 2]          # frame of tie track k's only box, in file order
UNKNOWN_IMAGE = 777777777


def video_of(motif):
    return 10 * (MOTIFS.index(motif) + 1)


def frame_images(motif):
    """Image ids of the motif's video in frame order."""
    return [x * 8 + MOTIFS.index(motif) for x in BASE_IDS]


def ground_truth(n_fill_images=0, seed=0):
    """One video per motif, each with the same five ground-truth tracks (the
    ``ties`` video: one-frame tracks under three of the tied detections as
    well; the ``dup_frame`` video: the only ground truth of category 9), and
    the filler video when asked for.  The image list is shuffled."""
    cats = [{"id": 1, "name": "a", "frequency": "f"},
            {"id": 2, "name": "b", "frequency": "c"},
            {"id": 3, "name": "c", "frequency": "r"},
            {"id": 4, "name": "d", "frequency": "f", "merged": [{"id": 5}]},
            {"id": 5, "name": "e", "frequency": "c"},
            {"id": 6, "name": "f", "frequency": "r"},
            {"id": 7, "name": "g", "frequency": "c"},
            {"id": 9, "name": "h", "frequency": "f"}]
    videos, images, tracks, anns = [], [], [], []

    def add_gt(tid, cat, vid, ims, box):
        tracks.append({"id": tid, "category_id": cat, "video_id": vid})
        for im in ims:
            anns.append({"id": len(anns) + 1, "image_id": im, "track_id": tid,
                         "category_id": cat, "bbox": list(box), "area": box[2] * box[3],
                         "visibility": 1.0, "out_of_frame": False})

    for m in MOTIFS:
        vid, im = video_of(m), frame_images(m)
        videos.append({"id": vid, "name": "v%d" % vid, "neg_category_ids": [3],
                       "not_exhaustive_category_ids": [2]})
        for f, i in enumerate(im):
            images.append({"id": i, "video_id": vid, "frame_index": 30 * f,
                           "neg_category_ids": [3], "not_exhaustive_category_ids": [2]})
        add_gt(100 * vid + 1, 1, vid, im, G1)
        add_gt(100 * vid + 2, 2, vid, im[:3], G2A)
        add_gt(100 * vid + 3, 2, vid, im[:10], G2B)
        add_gt(100 * vid + 4, 5, vid, im[2:9], G4)
        add_gt(100 * vid + 5, 7, vid, im[:8], G7)
        if m == "ties":
            for k in (0, 2, 4):
                add_gt(100 * vid + 10 + k, 1, vid, [im[TIE_FRAMES[k]]], _tie_box(k))
        if m == "dup_frame":
            add_gt(100 * vid + 6, 9, vid, im[:4], [800, 600, 30, 30])
    if n_fill_images:
        videos.append({"id": FILL_VIDEO, "name": "fill", "neg_category_ids": [],
                       "not_exhaustive_category_ids": []})
        for j in range(n_fill_images):
            images.append({"id": FILL_IMG0 + 2 * j, "video_id": FILL_VIDEO, "frame_index": j,
                           "neg_category_ids": [], "not_exhaustive_category_ids": []})
        add_gt(100 * FILL_VIDEO + 1, 1, FILL_VIDEO,
               [FILL_IMG0 + 2 * j for j in range(min(3, n_fill_images))], [10, 10, 15, 15])
    rng = np.random.default_rng([seed, 1])
    images = [images[i] for i in rng.permutation(len(images))]
    return {"info": {"description": "prediction rules"}, "images": images, "videos": videos,
            "tracks": tracks, "annotations": anns, "categories": cats}


def _tie_box(k):
    return [100 + 60 * k, 500, 50, 50]


def _shift(box, dx, dy=0):
    return [box[0] + dx, box[1] + dy, box[2], box[3]]


class _Ctx:
    """What a motif writes into: boxes in file order, named tracks and boxes."""

    def __init__(self, motif, max_dets, base, wide, names):
        self.motif, self.m, self.wide = motif, max_dets, wide
        self.vid, self.im = video_of(motif), frame_images(motif)
        self.base, self.names = base, names
        self.recs = []                # (part, prediction dict, box name)

    def track(self, name, tid=None):
        if tid is None:
            self.base[0] += 1
            tid = self.base[0]
        self.names["tracks"][self.motif + "." + name] = tid
        return tid

    def box(self, tid, cat, frame, box, score, part=1, name=None):
        self.recs.append((part, {"image_id": self.im[frame], "category_id": cat,
                                 "bbox": list(box), "score": score, "track_id": tid,
                                 "video_id": self.vid},
                          None if name is None else self.motif + "." + name))

    def single(self, cat, frame, box, score, part=1):
        """A track of one box that no test names."""
        self.base[0] += 1
        self.box(self.base[0], cat, frame, box, score, part)

    def shuffle(self, seed):
        rng = np.random.default_rng([seed, 2, MOTIFS.index(self.motif)])
        self.recs = [self.recs[i] for i in rng.permutation(len(self.recs))]


def _ties(c):
    # file order = TIE_FRAMES order; tracks 0, 2, 4 sit on a one-frame ground truth
    # (ids handed out in another order than the file's)
    tid = {k: c.track("t%d" % k) for k in (2, 4, 0, 3, 1)}
    for k, fr in enumerate(TIE_FRAMES):
        c.box(tid[k], 1, fr, _tie_box(k), 0.5)
    mean = c.track("mean")
    c.box(mean, 1, 5, [700, 500, 50, 50], 0.25)
    c.box(mean, 1, 6, [700, 500, 50, 50], 0.75)


def _dup_frame(c):
    t = c.track("first2")             # 3 frames, len 4: the first one doubled
    c.box(t, 2, 0, G2A, 0.9)
    c.box(t, 2, 0, _shift(G2A, -10, -10), 0.5)
    c.box(t, 2, 1, _shift(G2A, 1, 1), 0.9)
    c.box(t, 2, 2, G2A, 0.9)
    t = c.track("mid2")               # 10 frames, len 11: frame 5 doubled
    for f in range(10):
        c.box(t, 2, f, _shift(G2B, f % 3), 0.8)
    c.box(t, 2, 5, _shift(G2B, 40, 30), 0.3)
    t = c.track("last2")              # 2 frames, len 3: the last one doubled
    c.box(t, 1, 9, G1, 0.7)
    c.box(t, 1, 10, _shift(G1, 3), 0.7)
    c.box(t, 1, 10, _shift(G1, 30, 5), 0.6)
    t = c.track("only3")              # duplicates only: one frame, len 3
    for j in range(3):
        c.box(t, 1, 11, _shift(G1, 7 * j, j), 0.4 + 0.1 * j)
    c.shuffle(c.m)


def _votes(c):
    t = c.track("zero_among")         # mean 0.6 with the two zero-area boxes, 0.9 without
    c.box(t, 1, 0, G1, 0.9)
    c.box(t, 1, 1, [100, 100, 0, 50], 0.1)
    c.box(t, 1, 2, _shift(G1, 2), 0.9)
    c.box(t, 1, 3, [100, 100, 50, 0], 0.5)
    t = c.track("inf_neg")
    c.box(t, 2, 0, [300, 50, 1e200, 1e200], 0.2)
    c.box(t, 2, 1, [300, 50, -5, 10], 0.4)
    c.box(t, 2, 2, G2A, 0.6)
    t = c.track("none_valid")         # keeps its entry in track_scores, has no row
    c.box(t, 1, 4, [100, 100, 0, 50], 0.3)
    c.box(t, 1, 5, [100, 100, -5, 10], 0.7)
    t = c.track("unknown_cat")
    for f in (4, 5, 6):
        c.box(t, 42, f, [5, 5, 50, 50], 0.8)
    t = c.track("merged_away")        # predicted as 5, evaluated as 4
    for f in range(2, 9):
        c.box(t, 5, f, _shift(G4, 1, 1), 0.85 if f % 2 else 0.65)
    c.shuffle(c.m)


def _cut(c):
    m = c.m
    long_, l2 = c.track("long"), c.track("loses_one")
    # frame 0 (first seen): max_dets + 1 boxes, the lowest is `long`'s first box in the file
    c.box(long_, 2, 0, G2B, 0.05, part=0, name="long0")
    for k in range(m):
        c.single(1, 0, [10 + 40 * k, 600, 30, 30], 0.30 + 0.01 * k, part=0)
    # frame 1: exactly max_dets boxes
    c.box(long_, 2, 1, _shift(G2B, 1), 0.6, name="long1")
    for k in range(m - 1):
        c.single(1, 1, [10 + 40 * k, 600, 30, 30], 0.20 + 0.01 * k)
    # frame 2: max_dets + 2 boxes; a zero-area and an unknown-category box on top
    c.box(c.track("zero_hi"), 1, 2, [100, 100, 0, 50], 0.99)
    c.box(c.track("unknown_hi"), 42, 2, [100, 100, 50, 50], 0.98)
    c.box(long_, 2, 2, _shift(G2B, 2), 0.7)
    for k in range(m - 3):
        c.single(1, 2, [10 + 40 * k, 600, 30, 30], 0.40 + 0.01 * k)
    c.box(c.track("lost_all"), 1, 2, _shift(G1, 1), 0.03)
    c.box(l2, 1, 2, G1, 0.02)
    for f in (4, 5):
        c.box(long_, 2, f, _shift(G2B, f), 0.9 if f == 4 else 0.5)
        c.box(l2, 1, f, G1, 0.5)
    # frame 3 (last seen): max_dets + 1 boxes, two equal scores at the cut
    c.box(long_, 2, 3, _shift(G2B, 3), 0.8, part=2)
    for k in range(m - 2):
        c.single(1, 3, [10 + 40 * k, 600, 30, 30], 0.50 + 0.01 * k, part=2)
    c.box(c.track("tie_keep"), 1, 3, [700, 600, 30, 30], 0.1, part=2)
    c.box(c.track("tie_drop"), 1, 3, [740, 600, 30, 30], 0.1, part=2)


def _ids(c):
    zero, after = c.track("zero", 0), c.track("after_zero")
    for f in range(12):
        c.box(zero, 1, f, G1, 0.9)
        c.box(after, 1, f, G1, 0.8)
    t = c.track("w31", 2 ** 31 if c.wide else None)
    for f in range(3):
        c.box(t, 2, f, G2A, 0.7)
    t = c.track("w40", 2 ** 40 + 5 if c.wide else None)
    for f in range(3, 8):
        c.box(t, 7, f, G7, 0.6)
    t = c.track("neg_listed")         # no ground truth of category 3, listed: kept
    for f in (8, 9):
        c.box(t, 3, f, [10, 10, 20, 20], 0.95)
    c.box(c.track("unlisted"), 6, 10, [5, 5, 50, 50], 0.99)
    # category 9 has ground truth, in another video only
    c.box(c.track("elsewhere", 2 ** 31 + 1 if c.wide else None), 9, 11, [800, 600, 30, 30], 0.97)
    c.shuffle(c.m)


_BUILD = {"ties": _ties, "dup_frame": _dup_frame, "votes": _votes, "cut": _cut, "ids": _ids}


class RuleSet:
    """gt / preds: JSON-shaped; motif[i]: the motif of prediction i ("fill"
    for a filler); tracks / boxes: name -> track id / file position."""

    def __init__(self, gt, preds, motif, tracks, boxes, max_dets):
        self.gt, self.preds, self.motif = gt, preds, motif
        self.tracks, self.boxes, self.max_dets = tracks, boxes, max_dets

    def columns(self):
        return GTColumns.from_json(self.gt), DTColumns.from_json(self.preds)


def sized(n_boxes=None, n_tracks=None, n_images=None, max_dets=3, where="split",
          low_fillers=None, motif_base=10 ** 6, wide=False, motifs=MOTIFS, seed=0):
    """Every motif once, designed for `max_dets`, padded to exactly `n_boxes`
    predictions (None: no padding), `n_tracks` track ids and `n_images`
    ground-truth images.  The fillers are tracks of distinct scores in the
    filler video: one box each on an image of its own unless the counts ask
    for longer tracks or fewer images.  `where`: the motifs' boxes come
    "first" or "last" in the file or "split" around the fillers (a motif box
    at position 0 and at n - 1).  Filler track ids: the first `low_fillers`
    (None: all) 1, 2, ... below the motif tracks' (`motif_base` + 1 ...), the
    rest above them.  `wide`: the ids motif's tracks at 2^31 and 2^40."""
    names = {"tracks": {}, "boxes": {}}
    base = [motif_base]
    recs = []
    for mo in motifs:
        c = _Ctx(mo, max_dets, base, wide, names)
        _BUILD[mo](c)
        recs += [(part, mo, p, name) for part, p, name in c.recs]
    recs.sort(key=lambda r: r[0])                         # (stable)
    n_motif = len(recs)
    motif_tracks = len({r[2]["track_id"] for r in recs})
    motif_images = len(MOTIFS) * len(BASE_IDS)
    n_fill = 0 if n_boxes is None else n_boxes - n_motif
    if n_fill < 0:
        raise ValueError("the motifs alone hold %d boxes" % n_motif)
    fill_tracks = n_fill if n_tracks is None else n_tracks - motif_tracks
    fill_images = n_fill if n_images is None else n_images - motif_images
    if n_fill and not (0 < fill_tracks <= n_fill and 0 < fill_images):
        raise ValueError("counts do not fit")
    low = fill_tracks if low_fillers is None else low_fillers
    if not 0 <= low <= fill_tracks or low >= motif_base:
        raise ValueError("low_fillers does not fit")
    fill = []
    j = 0
    for t in range(fill_tracks):
        tid = 1 + t if t < low else motif_base + 10 ** 5 + t
        for _ in range(n_fill // fill_tracks + (t < n_fill % fill_tracks)):
            # distinct, exact scores; a track's boxes on consecutive images
            fill.append((1, "fill", {"image_id": FILL_IMG0 + 2 * (j % fill_images),
                                     "category_id": 1,
                                     "bbox": [10 + 20 * (j % 50), 10 + 20 * (j // 50 % 30), 15, 15],
                                     "score": (j + 1) / 8192.0, "track_id": tid,
                                     "video_id": FILL_VIDEO}, None))
            j += 1
    if where == "first":
        recs = recs + fill
    elif where == "last":
        recs = fill + recs
    else:
        assert where == "split", where
        recs = recs[:n_motif // 2] + fill + recs[n_motif // 2:]
    for i, r in enumerate(recs):
        if r[3] is not None:
            names["boxes"][r[3]] = i
    return RuleSet(ground_truth(fill_images if n_fill else 0, seed), [r[2] for r in recs],
                   [r[1] for r in recs], names["tracks"], names["boxes"], max_dets)


def clash_inputs(s):
    """name -> prediction list derived from `s` (which holds the cut motif):
    cat_cut   a second category on a box the cut removes (no error at
              s.max_dets), cat_stay the same on a box that stays
    vid_cut   a second video on a box the cut removes (still an error:
              ensure_unique_track_ids looks at every box)
    unknown_image  a prediction on an image the ground truth does not hold"""
    out = {}
    for name, box, key, value in (("cat_cut", "cut.long0", "category_id", 1),
                                  ("cat_stay", "cut.long1", "category_id", 1),
                                  ("vid_cut", "cut.long0", "video_id", video_of("ids"))):
        preds = copy.deepcopy(s.preds)
        preds[s.boxes[box]][key] = value
        out[name] = preds
    preds = copy.deepcopy(s.preds)
    preds.insert(len(preds) // 2, {"image_id": UNKNOWN_IMAGE, "category_id": 1,
                                   "bbox": [1, 1, 10, 10], "score": 0.5,
                                   "track_id": max(p["track_id"] for p in preds) + 1,
                                   "video_id": video_of("cut")})
    out["unknown_image"] = preds
    return out


# the sets the reference's class API was recorded on (predrules.npz): name -> max_dets
RECORDED = {"m3": 3, "m8": 8}


def recorded_set(name):
    return sized(max_dets=RECORDED[name], wide=True)


# ---------------------------------------------------------------------------
# what a set must hold for its motifs to mean anything
# ---------------------------------------------------------------------------
class Outcome:
    """What the rules made of a set: post_cut (file positions in list order),
    track_scores {track id: score}, rows {track id: (len, frame image ids)} of
    the tracks that reach the table, cells {(video, category): track ids in
    cell order}.  Built from the reference's recording (from_recording) or
    from flatten.py's tables (from_flat)."""

    def __init__(self, post_cut, track_scores, rows, cells):
        self.post_cut, self.track_scores = [int(x) for x in post_cut], track_scores
        self.rows, self.cells = rows, cells

    @classmethod
    def from_recording(cls, post_cut, rec):
        return cls(post_cut, {int(t): v for t, v in rec["track_scores"].items()},
                   {int(t): (r["len"], list(r["frame_images"])) for t, r in rec["tracks"].items()},
                   {tuple(c["key"]): list(c["dt_ids"]) for c in rec["cells"]})

    @classmethod
    def from_flat(cls, post_cut, f):
        rows, cells = {}, {}
        off = np.asarray(f.dt_frame_off)
        pos = np.asarray(f.dt_frame_pos)
        for k in range(f.n_cells):
            v = int(f.cell_unit[k])
            ids = []
            for i in range(int(f.cell_dt_off[k]), int(f.cell_dt_off[k + 1])):
                ims = f.tl_image_id[f.tl_vid_start[v] + pos[off[i]:off[i + 1]]]
                rows[int(f.dt_id[i])] = (int(f.dt_len[i]), [int(x) for x in ims])
                ids.append(int(f.dt_id[i]))
            if ids:
                cells[int(f.vid_ids[v]), int(f.cat_ids[int(f.cell_cat[k])])] = ids
        return cls(post_cut, {int(t): v for t, v in f.track_scores.items()}, rows, cells)


def check_situations(s, o):
    """Every motif of `s` holds what it names, given the outcome `o`."""
    t, m = s.tracks, s.max_dets
    kept = set(o.post_cut)

    def boxes_of(tid):
        return [i for i, p in enumerate(s.preds) if p["track_id"] == tid]

    # dup_frame: len counts boxes, the frame list images
    for name, want in (("first2", (4, 3)), ("mid2", (11, 10)), ("last2", (3, 2)),
                       ("only3", (3, 1))):
        n, frames = o.rows[t["dup_frame." + name]]
        assert (n, len(frames)) == want, (name, n, frames)
        assert len(set(frames)) == len(frames)
    # votes: invalid boxes move the score and nothing else
    assert o.track_scores[t["votes.zero_among"]] == np.mean([0.9, 0.1, 0.9, 0.5])
    assert o.track_scores[t["votes.zero_among"]] != 0.9
    assert o.rows[t["votes.zero_among"]][0] == 2
    assert o.rows[t["votes.inf_neg"]][0] == 1
    for name in ("votes.none_valid", "votes.unknown_cat", "cut.zero_hi", "cut.unknown_hi",
                 "ids.unlisted", "ids.elsewhere"):
        assert t[name] in o.track_scores and t[name] not in o.rows, name
    assert t["votes.merged_away"] in o.cells[video_of("votes"), 4]
    assert t["ids.neg_listed"] in o.cells[video_of("ids"), 3]
    assert o.cells[video_of("ids"), 1][:2] == [0, t["ids.after_zero"]]
    # cut: a track that loses its first box, one that loses all, a valid box
    # displaced by the zero-area and the unknown-category box, the tie at the cut
    long_boxes = boxes_of(t["cut.long"])
    assert long_boxes[0] == s.boxes["cut.long0"] == min(
        i for i, mo in enumerate(s.motif) if mo == "cut") and long_boxes[0] not in kept
    assert all(i in kept for i in long_boxes[1:]) and o.rows[t["cut.long"]][0] == 5
    scores = [s.preds[i]["score"] for i in long_boxes[1:]]
    assert o.track_scores[t["cut.long"]] == np.mean(scores) != np.mean(
        [s.preds[i]["score"] for i in long_boxes])
    assert t["cut.lost_all"] not in o.track_scores and t["cut.lost_all"] not in o.rows
    assert o.rows[t["cut.loses_one"]][0] == 2 and o.track_scores[t["cut.loses_one"]] == 0.5
    lost = boxes_of(t["cut.lost_all"])[0]
    on_image = [i for i in kept if s.preds[i]["image_id"] == s.preds[lost]["image_id"]]
    valid = [i for i in on_image if s.preds[i]["category_id"] != 42
             and 0 < s.preds[i]["bbox"][2] * s.preds[i]["bbox"][3] < float("inf")]
    assert len(on_image) == m and len(valid) == m - 2
    assert boxes_of(t["cut.zero_hi"])[0] in kept and lost not in kept
    assert min(s.preds[i]["score"] for i in valid) > s.preds[lost]["score"]
    assert boxes_of(t["cut.tie_keep"])[0] in kept and boxes_of(t["cut.tie_drop"])[0] not in kept
    per_image = {}
    for i, p in enumerate(s.preds):
        if s.motif[i] == "cut":
            per_image.setdefault(p["image_id"], []).append(i)
    counts = sorted(len(v) for v in per_image.values())
    assert m in counts and m + 1 in counts and m + 2 in counts
    # ties: six equal scores, ordered by first appearance in the visiting order
    tie = [t["ties.t%d" % k] for k in range(5)] + [t["ties.mean"]]
    assert all(o.track_scores[x] == 0.5 for x in tie)
    in_cell = [x for x in o.cells[video_of("ties"), 1] if x in tie]
    file_order = sorted(tie, key=lambda x: boxes_of(x)[0])
    assert len(in_cell) == 6 and in_cell != file_order and in_cell != sorted(tie) \
        and file_order != sorted(tie)
    ids = [im["id"] for v in sorted({x["video_id"] for x in s.gt["images"]})
           for im in s.gt["images"] if im["video_id"] == v]
    visit = {im: k for k, im in enumerate(set(ids) & set(ids))}
    assert in_cell == sorted(tie, key=lambda x: min(
        visit[s.preds[i]["image_id"]] for i in boxes_of(x)))


def tie_order(s, image_ids):
    """The `ties` tracks of `s` by the first appearance of a box of theirs in
    the CPython set iteration of `image_ids` (in the order the reference
    collects them: flatten.video_images)."""
    ids = [int(i) for i in image_ids]
    visit = {im: k for k, im in enumerate(set(ids) & set(ids))}
    tie = [s.tracks["ties.t%d" % k] for k in range(5)] + [s.tracks["ties.mean"]]
    return sorted(tie, key=lambda x: min(visit[p["image_id"]] for p in s.preds
                                         if p["track_id"] == x))
