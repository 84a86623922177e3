"""``TaoEval``: track-level federated mAP (3D IoU) on the GPU.  Same
constructor, methods, public state and logged lines as the reference class
(tao_amodal/evaluation/tao_amodal/eval.py:120-717); the per-(video, category)
Python loops are replaced by the HIP pipeline over the non-empty cells.

``iou_type="segm"`` (which the reference accepts but cannot run) evaluates
mask tracks: the three ``iou_3d_type`` metrics over run-length masks
(csrc/track_mask_iou.hip); a params.vid_ids subset and a multi-GPU run raise
NotImplementedError there.
"""
import logging
from collections import OrderedDict
from collections.abc import Mapping

import numpy as np

from .. import _core
from . import followers
from .._core import (N_REC, N_THR, CellView, GpuRun, LazyIous, LazyPointers,
                     EvalConstants,
                     masked_mean, now, operating_points, summaries, timed)
from .results import TaoResults
from .tao import Tao


class Params:
    def __init__(self, iou_type, iou_3d_type="3d_iou"):
        """Params of the Tao evaluation (reference eval.py:720-757)."""
        self.vid_ids = []
        self.cat_ids = []
        self.iou_thrs = np.linspace(
            0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
        self.rec_thrs = np.linspace(
            0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01) + 1), endpoint=True)
        self.max_dets = 300
        self.area_rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2],
                         [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2],
                         [0 ** 2, 1e5 ** 2]]
        self.area_rng_lbl = ["all", "small", "medium", "large",
                             "highly-and-partially-occluded"]
        self.time_rng = [[0, 1e5], [0, 3], [3, 10], [10, 1e5]]
        self.time_rng_lbl = ["all", "short", "medium", "long"]
        self.use_cats = 1
        self.vid_count_lbl = ["r", "c", "f"]
        self.iou_type = iou_type
        self.iou_3d_type = iou_3d_type


class _EvalVids(Mapping):
    """``eval_vids[(v, c, a, t)]`` of the reference, rebuilt when read."""

    def __init__(self, view, n_vid, n_cat, n_area, n_time):
        self.view = view
        self.shape = (n_vid, n_cat, n_area, n_time)

    def __len__(self):
        return int(np.prod(self.shape))

    def __iter__(self):
        V, C, A, T = self.shape
        return ((v, c, a, t) for c in range(C) for a in range(A)
                for t in range(T) for v in range(V))

    def __getitem__(self, key):
        v, c, a, t = key
        V, C, A, T = self.shape
        if not (0 <= v < V and 0 <= c < C and 0 <= a < A and 0 <= t < T):
            raise KeyError(key)
        k = self.view.cell_of(v, c)
        if k is None:
            return None
        e = self.view.entry(k, a * T + t)
        e["area_rng"], e["time_rng"] = e.pop("rng")
        return e


class TaoEval:
    def __init__(self, tao_gt, tao_dt, logger=None, iou_type="bbox",
                 iou_3d_type="3d_iou", device=None, dist=None):
        """``dist`` (evaluation/_dist.Ctx): this process is one rank of a
        multi-GPU evaluation, tao_gt / tao_dt are its share (videos of one
        block of the sorted video ids)."""
        if not logger:
            self.logger = logging.getLogger("tao.eval")
        elif isinstance(logger, str):
            self.logger = logging.getLogger(logger)
        else:
            self.logger = logger
        if iou_type not in ["bbox", "segm"]:
            raise ValueError("iou_type: {} is not supported.".format(iou_type))
        if isinstance(tao_gt, Tao):
            self.tao_gt = tao_gt
        elif isinstance(tao_gt, str):
            self.tao_gt = Tao(tao_gt)
        else:
            raise TypeError("Unsupported type {} of tao_gt.".format(tao_gt))
        if isinstance(tao_dt, TaoResults):
            self.tao_dt = tao_dt
        elif isinstance(tao_dt, (str, list)):
            self.tao_dt = TaoResults(self.tao_gt, tao_dt)
        else:
            raise TypeError("Unsupported type {} of tao_dt.".format(tao_dt))
        self.device = device if dist is None else dist.device
        self.dist = dist
        self.eval_vids = {}
        self.eval = {}
        self.params = Params(iou_type=iou_type, iou_3d_type=iou_3d_type)
        self.results = OrderedDict()
        self.ious = {}
        self.params.vid_ids = sorted(self.tao_gt.get_vid_ids())
        self.params.cat_ids = sorted(self.tao_gt.get_cat_ids())
        self.flat = self.tao_dt.flat
        self._run = None
        self._cat_pos = None
        self._reset_analyses()
        self._gt_columns = None

    def _reset_analyses(self):
        """The caches of the analyses on request: they hold results of one evaluate()."""
        self._error_types, self._error_impact, self._confusion = {}, {}, {}
        self._association, self._occlusions, self._identity = {}, {}, {}
        self._hota = {}
        self._clear = {}

    # ------------------------------------------------------------ stages
    def evaluate(self, show_progress=False):
        self.logger.info("Running per video evaluation.")
        self.logger.info("Evaluate annotation type *{}*".format(self.params.iou_type))
        segm = self.params.iou_type == "segm"
        if segm and self.dist is not None:
            raise NotImplementedError("multi-GPU runs evaluate iou_type='bbox'")
        if self.params.iou_3d_type not in ("3d_iou", "avg_iou", "imagenetvid"):
            raise ValueError("Unknown iou_3d_type %r" % self.params.iou_3d_type)
        self.params.vid_ids = list(np.unique(self.params.vid_ids))
        constants = EvalConstants(self.params, Params(self.params.iou_type), "tao")
        # params.vid_ids / cat_ids subsets (reference eval.py:178-233)
        from .._core import restrict_to_params
        gt_cols, dt_cols, self._cat_pos = restrict_to_params(
            self.tao_gt.columns, self.tao_dt.columns_dt, "video",
            self.params.vid_ids, self.params.cat_ids, bool(self.params.use_cats))
        subset = gt_cols is not self.tao_gt.columns
        if subset and segm:
            raise NotImplementedError("iou_type='segm' with a params.vid_ids subset")
        if subset:
            if len(gt_cols.ann_id) == 0:
                raise ValueError("Found no groundtruth annotations for given params")
            if len(dt_cols) == 0:
                raise ValueError("Found no predicted annotations for given params")
            if self.dist is not None:
                raise NotImplementedError("params.vid_ids subsets in a multi-GPU run")
        if segm:
            # the host statement of the tables: it also names the annotation
            # every frame comes from (*_frame_ann), whose mask the frame takes
            from ... import flatten
            self.flat = flatten.flatten_tao(
                gt_cols, dt_cols, self.tao_dt.max_dets,
                use_cats=bool(self.params.use_cats))
            with timed("masks"):
                self.flat.masks = self._masks(self.flat)
        elif not self.params.use_cats:
            # class-agnostic cells (reference eval.py:257-260,293-303)
            from ... import flatten
            self.flat = flatten.flatten_tao(
                gt_cols, dt_cols, self.tao_dt.max_dets, use_cats=False)
        elif subset:
            from ... import flatten_dev
            self.flat = flatten_dev.flatten_tao(gt_cols, dt_cols, self.tao_dt.max_dets,
                                                device=self.device)
        flat = self.flat
        if self.dist is not None:
            from .._dist import DistRun
            self._run = DistRun(flat, self.dist, self.params.iou_3d_type,
                                constants=constants)
        else:
            self._run = GpuRun(flat, self.device, self.params.iou_3d_type,
                               constants=constants)
        self._reset_analyses()
        self._gt_columns = gt_cols      # the annotation rows the tables' frames name
        self._run.evaluate()
        P = self.params
        rngs = [(a, t) for a in P.area_rng for t in P.time_rng]
        view = CellView(self._run, flat.vid_ids, -1, "video_id", "rng", rngs)
        view.cat_pos = self._cat_pos
        cats = P.cat_ids if P.use_cats else [-1]
        self.ious = LazyIous(view, P.vid_ids, cats)
        self.eval_vids = _EvalVids(view, len(P.vid_ids), len(cats),
                                   len(P.area_rng), len(P.time_rng))

    def _masks(self, flat):
        """One run-length mask per frame of the track tables (iou_type="segm"):
        a ground-truth frame takes Tao.ann_to_rle of its annotation; a
        prediction its "segmentation" (polygons, uncompressed or compressed
        RLE), or the polygon of its box where it has none (reference
        results.py:67-68).  Polygons are rasterised at the image's size."""
        from ...masks import MaskBatch
        imgs = self.tao_gt.imgs
        anns = self.tao_gt.dataset["annotations"]
        raw = self.tao_dt.raw_results

        def gt_items():
            for row in np.asarray(flat.gt_frame_ann).tolist():
                a = anns[row]
                im = imgs[a["image_id"]]
                yield a["segmentation"], im["height"], im["width"]

        def dt_items():
            for row in np.asarray(flat.dt_frame_ann).tolist():
                r = raw[row]
                im = imgs[r["image_id"]]
                if "segmentation" in r:
                    seg = r["segmentation"]
                else:
                    x1, y1, w, h = r["bbox"]
                    x2, y2 = x1 + w, y1 + h
                    seg = [[x1, y1, x1, y2, x2, y2, x2, y1]]
                yield seg, im["height"], im["width"]

        out = {}
        for side, items in (("gt", gt_items()), ("dt", dt_items())):
            batch = MaskBatch()
            batch.add_many(items)       # polygons: one native call, all cores
            out[side] = batch.arrays()
            batch.close()
        return out

    @property
    def near_threshold_pairs(self):
        """Track pairs whose 3D IoU the frame-order guard recomputed in the
        reference's set order (it sat within the reordering bound of a
        comparison of the match).  Reads a device counter: synchronises."""
        if self._run is None:
            return 0
        return self._run.engine.guarded_pairs(self._run.dp, self._run.ws)

    def accumulate(self):
        self.logger.info("Accumulating evaluation results.")
        if self._run is None:
            self.logger.warning("Please run evaluate first.")
            return
        self._run.accumulate()
        # frame-order guard: the listed pairs are recomputed one per thread in
        # the reference's set order -- rare on real data (an IoU within the
        # reordering bound of a comparison); many of them (identical tracks,
        # avg_iou on integer boxes with exact rival ties) make the pass slow
        # without making it wrong: say so
        near, n_iou = self._run.near_threshold_pairs, getattr(self._run.dp, "n_iou", 0)
        if near > 4096 and near * 100 > n_iou:
            logging.getLogger("taoamd.guard").warning(
                "%d of %d track pairs went through the frame-order guard", near, n_iou)
        P = self.params
        A, T = len(P.area_rng), len(P.time_rng)
        K = len(P.cat_ids) if P.use_cats else 1
        precision, recall = self._run.precision, self._run.recall
        if self._cat_pos is not None:
            # the category axis in the order of params.cat_ids
            precision = np.ascontiguousarray(precision[:, :, self._cat_pos])
            recall = np.ascontiguousarray(recall[:, self._cat_pos])
        self.eval = {
            "params": P,
            "counts": [len(P.iou_thrs), len(P.rec_thrs), K, A, T],
            "date": now(),
            "precision": precision.reshape(len(P.iou_thrs), len(P.rec_thrs), K, A, T),
            "recall": recall.reshape(len(P.iou_thrs), K, A, T),
            "dt_pointers": LazyPointers(self._run, A * T, (A, T), self._cat_pos),
        }

    # what the shared bodies of the on-request analyses (_core) ask of the level
    _level = " track"

    @staticmethod
    def _rng_text(lbl):
        return "{}/{}".format(*lbl)

    def _rng_lbl(self):
        """The (area label, time label) of every range; an index where the
        labels run out."""
        P = self.params

        def lbl(names, i):
            return names[i] if i < len(names) else str(i)
        return [(lbl(P.area_rng_lbl, a), lbl(P.time_rng_lbl, t))
                for a in range(len(P.area_rng)) for t in range(len(P.time_rng))]

    def _cats(self):
        return self.tao_gt.cats

    def _dt_ids(self):
        return np.asarray(self._run.flat.dt_id)

    def score_at_recall(self):
        """eval["scores"][T, R, K, area range, time range], pycocotools' table
        beside eval["precision"]: the score of the track at which recall first
        reaches each recall threshold (-1: no evaluated ground truth, 0: never
        reached).  Computed on the first call, from what accumulate() left on
        the device."""
        return _core.score_at_recall(self)

    def operating_points(self, iou_thr, recall, rng=("all", "all")):
        """{category id: track score threshold} at which the category reaches
        `recall` at `iou_thr` in the (area, time) range labelled `rng`, read
        from eval["scores"] (score_at_recall() first)."""
        if "scores" not in self.eval:
            raise RuntimeError("Please run score_at_recall() first.")
        P = self.params
        aidx, tidx = P.area_rng_lbl.index(rng[0]), P.time_rng_lbl.index(rng[1])
        cats = P.cat_ids if P.use_cats else [-1]
        return operating_points(self.eval["scores"][..., aidx, tidx], P.iou_thrs,
                                P.rec_thrs, cats, iou_thr, recall)

    def error_types(self, iou_thr=0.5, bg_thr=0.1, per_detection=False):
        """Why a detection track is no true positive, per (area, time) range
        and category, at the IoU threshold `iou_thr` (one of params.iou_thrs;
        the foreground threshold tf = min(iou_thr, 1 - 1e-10)) and the
        background threshold `bg_thr` (0 <= bg_thr < tf): LVISEval.error_types()
        rule for rule on tracks and their 3D IoU.  No counterpart in the
        reference.  Callable after evaluate(), computed on the device on request
        (csrc/track_error_types.hip), cached per (iou_thr, bg_thr).

        Rows are the detection tracks that survived the max_dets cut and the
        federated filter.  With s the largest 3D IoU of a track with the
        ground-truth tracks of ITS category in its video that the range
        evaluates (0 if none; taken from the IoU matrix the match read) and o
        the same over the video's other categories, a (track, range) pair is
        the first of: TP (matched to an evaluated ground truth), IGNORED
        (matched to an ignored one, or unmatched and itself outside the range:
        a not-exhaustive category, or an area / length outside the range's
        windows), DUP (unmatched, s >= tf: the ground truth is held by another
        track), LOC (bg_thr <= s < tf), CLS (o >= tf), BOTH (bg_thr <= o < tf),
        BKG.  Per evaluated ground-truth track: `evaluated`, `missed` (no
        detection track is matched to it), `missed_loc` (missed, and the best
        same-category ground truth -- the first in table order among equal
        IoUs -- of at least one LOC track).

        Returns {"types": the 7 names, "dt_counts": int64[n_rng, K, 7],
        "gt_counts": int64[n_rng, K, 3], "rng_lbl": the (area label, time
        label) of every range} with n_rng = areas x durations in the order of
        eval["precision"]'s last two axes flattened, the category axis in the
        order of params.cat_ids, and with per_detection=True "dt_type": (ids,
        types) = the rows' track ids and uint8[n, n_rng].

        The table follows the match itself: a track matched to a ground truth
        whose id is the "unmatched" sentinel counts as TP here, whereas
        accumulate(), like the reference, sees it as unmatched.  Not available:
        iou_type="segm", use_cats = 0, an iou_3d_type other than "3d_iou", more
        than one block of edited constants, multi-GPU runs."""
        return _core.error_types(self, iou_thr, bg_thr, per_detection)

    def error_lines(self, iou_thr=0.5, bg_thr=0.1):
        """error_types() as a small text table: a line per (area, time) range,
        the seven types and the three ground-truth counts summed over the
        categories.  Returned, not printed."""
        return _core.error_lines(self, iou_thr, bg_thr)

    def error_impact(self, iou_thr=0.5, bg_thr=0.1):
        """The Track-AP each error type costs, per (area, time) range: TIDE's
        dAP (Bolya et al., ECCV 2020) on the table of error_types(iou_thr,
        bg_thr), LVISEval.error_impact() rule for rule on tracks.  For each of
        nine variants of the evaluation -- BASE and one fix each, a fix applied
        to BASE alone -- the precision table at `iou_thr` is computed once more
        on the device (csrc/track_error_types.hip for the links, csrc/
        error_impact.hip for the sweep), with accumulate()'s arithmetic.
        Callable after evaluate(), cached per (iou_thr, bg_thr).

        The fixes are LVISEval.error_impact()'s: CLS, LOC, BOTH, DUP, BKG, MISS,
        FP, FN; a CLS track is handed the ground-truth track of another
        category whose plan-less 3D IoU with it is greatest among those the
        range evaluates, a LOC track the best one of its own category by the
        IoU matrix the match read.  The exact rules are in
        include/tao_amodal_hip.h, section "error impact".

        Returns {"fixes": the nine names, "precision": float64[9, R, K, n_rng]
        (-1: nothing to evaluate, like eval["precision"]), "ap": float64[9,
        n_rng] = the mean of the precisions > -1 of each [R, K] slab, "dap":
        float64[8, n_rng] = ap[1:] - ap[0], "rng_lbl": the (area label, time
        label) of every range} with n_rng = areas x durations in the order of
        eval["precision"]'s last two axes flattened and the category axis in
        the order of params.cat_ids.  ap[0] is what summarize() reports as AP at
        `iou_thr`, except where a ground-truth track whose id is the
        "unmatched" sentinel holds a detection track (see error_types()).  Not
        available where error_types() is not, nor with more than 101 recall
        thresholds."""
        return _core.error_impact(self, iou_thr, bg_thr)

    def association(self, frame_thr=0.5, vis_rng=None, vis_lbl=None, per_track=False,
                    per_frame=False):
        """Which detection track follows a ground-truth track, frame by frame:
        coverage, ID switches, fragmentation, mostly-tracked / mostly-lost, and
        coverage split by the frames' visibility -- what error_types() cannot
        say about a LOC or missed ground-truth track (never found, handed from
        id to id, or lost when it became occluded).  No counterpart in the
        reference.  Callable after evaluate(), computed on the device on request
        (csrc/track_association.hip), cached per argument set.

        Rows are the tracks that survived the max_dets cut and the federated
        filter.  The candidates of a ground-truth track are the detection tracks
        of its video and category, whatever their flags.  On a frame of the
        ground truth, the best follower is the candidate with a box in that
        frame whose box IoU (pycocotools' bbIou, not crowd) with the ground
        truth's is greatest and at least `frame_thr`, a double in (0, 1] -- the
        best-scored one among equal IoUs; the frame is covered if there is one.
        Per ground-truth track: `frames`, `covered`, `ids` (distinct followers),
        `switches` (covered frames whose follower differs from that of the
        covered frame before), `fragments` (covered stretches of the track's own
        frame list), `primary` (the track that follows most frames, the
        best-scored among equal counts) and `primary_frames`.  Per category,
        over the ground-truth tracks that are not ignored: `tracks`, the sums of
        `frames`, `covered`, `ids`, `switches`, `fragments`, and `mostly_tracked`
        (covered >= 80 % of the frames), `mostly_lost` (< 20 %).  Per closed
        visibility window [lo, hi] (up to 8, they may overlap; default: the
        image level's all, highly-occluded, partially-occluded, highly-visible,
        highly-and-partially-occluded) and category: `frames`, `covered` and
        frames followed by the track's `primary`; a NaN visibility is in none.

        Returns {"columns": {"tracks": ..., "cat_counts": ..., "vis_counts":
        ...} (the column names), "cat_counts": int64[K, 8], "vis_counts":
        int64[n_vis, K, 3], "vis_rng", "vis_lbl", "frame_thr"} with the category
        axis in the order of params.cat_ids; with per_track=True "tracks":
        (ground-truth track ids, int64[n_gt, 7], `primary` as the detection
        track's id, -1 for none); with per_frame=True "frames": (frame_off
        int64[n_gt + 1], image ids, the best detection track's id per frame or
        -1, best_iou -- 0.0 where uncovered), frames of track i at frame_off[i]
        .. frame_off[i + 1].  It reads the track tables alone: the result does
        not depend on iou_3d_type, params.iou_thrs or the ranges.  Not available:
        iou_type="segm", use_cats = 0, multi-GPU runs."""
        return followers.association(self, frame_thr, vis_rng, vis_lbl, per_track, per_frame)

    def association_lines(self, frame_thr=0.5, vis_rng=None, vis_lbl=None):
        """association() as a small text table: the totals over the categories,
        then a line per visibility window with its frames, the covered ones and
        those the primary follower covers, in per cent.  Returned, not printed."""
        return followers.association_lines(self.association(frame_thr, vis_rng, vis_lbl))

    def occlusions(self, frame_thr=0.5, vis_rng=(0.0, 0.1), recover=3, len_edges=(1, 3, 6, 11),
                   per_track=False, per_episode=False):
        """Whether a ground-truth track's follower is KEPT while the object is
        hidden -- what association()'s coverage per visibility window, which
        counts every frame on its own, cannot say: a tracker that keeps the id
        across every occlusion and one that drops the object and re-acquires it
        under a new id have the same coverage.  No counterpart in the reference.
        Callable after evaluate(), computed on the device on request
        (csrc/track_occlusion.hip) from association(frame_thr)'s per-frame
        followers, cached per argument set.

        A frame of a ground-truth track is occluded when its visibility lies in
        the closed window `vis_rng` = (lo, hi); a NaN visibility is not.  An
        episode is a maximal run of occluded frames of the track's own frame
        list, `n` frames from frame `a` on.  `entry` is the follower of the frame
        before the run, `covered` the run's frames with a follower, `held` those
        followed by `entry`; `after` is the follower of the first covered frame
        among the `recover` (1 to 64) frames behind the run and `gap` the
        uncovered frames before it.  One outcome each, the first that applies:
        START (the run begins the track), UNFOLLOWED (nobody follows on entry),
        END (the run ends the track), KEPT (after == entry), SWITCHED (another
        track follows), LOST (none within `recover` frames).  Episodes are
        grouped by length: `len_edges`, up to 8 ascending lengths that start at
        1, bucket j holds len_edges[j] <= n < len_edges[j + 1], the last is open.
        The exact rules are in include/tao_amodal_hip.h, section "track-level
        occlusion episodes".

        Returns {"columns": {"counts": ..., "tracks": ..., "episodes": ...,
        "outcomes": ...} (the column and outcome names), "counts": int64[K, n_len,
        11] over the ground-truth tracks that are not ignored = episodes, frames,
        covered, held, start, unfollowed, end, kept, switched, lost, gap, with
        the category axis in the order of params.cat_ids, "len_edges", "len_lbl",
        "vis_rng", "frame_thr", "recover"}; with per_track=True "tracks":
        (ground-truth track ids, int64[n_gt, 4] = episodes, occluded frames,
        kept, switched + lost), ignored tracks included; with per_episode=True
        "episodes": (ground-truth track ids, first image ids, last image ids,
        int64[n_ep, 9] = ground-truth row, a, n, outcome, entry, after, gap,
        covered, held with entry and after as detection track ids, -1 for none),
        by ascending (row, a).  Not available: iou_type="segm", use_cats = 0,
        multi-GPU runs."""
        return followers.occlusions(self, frame_thr, vis_rng, recover, len_edges, per_track,
                                    per_episode)

    def occlusion_lines(self, frame_thr=0.5, vis_rng=(0.0, 0.1), recover=3,
                        len_edges=(1, 3, 6, 11)):
        """occlusions() as a small text table, the totals over the categories: a
        line per length bucket with its episodes, the kept / switched / lost
        shares of the episodes that have one of these three outcomes, and held /
        frames, in per cent.  Returned, not printed."""
        return followers.occlusion_lines(self.occlusions(frame_thr, vis_rng, recover, len_edges))

    def identity(self, frame_thr=0.5, per_track=False, score_thr=None):
        """IDF1, IDP and IDR (Ristani et al., ECCV 2016; TrackEval's Identity):
        the identity measure beside Track-AP.  association() is many-to-one --
        one detection track may be the primary of several ground-truth tracks,
        and a ground truth's covered frames may be spread over many ids; its
        switches and fragments are the symptoms, this is the cost.  Each
        ground-truth track may own ONE detection track and each detection track
        at most one ground truth: under that rule, how many frames can be
        explained?  A maximum-weight one-to-one assignment per (video, category),
        solved on the device on request (csrc/track_identity.hip).  Callable
        after evaluate(), cached per threshold.

        Rows are the tracks that survived the max_dets cut and the federated
        filter.  The weight of a pair of one video and category is its `share`:
        the frames of the ground truth on which the detection track has a box
        whose box IoU (pycocotools' bbIou, not crowd) with the ground truth's is
        at least `frame_thr`, a double in (0, 1].  Ground-truth tracks marked
        "ignore" take no part.  A detection track is set aside -- neither
        assigned nor counted -- if its greatest share with an ignored ground
        truth exceeds its greatest share with any other, or if it is marked
        "ignore unmatched" (a category that is not exhaustively annotated or
        absent in the video) and shares no frame with a ground truth that takes
        part.  `idtp` is the greatest sum of shares an assignment reaches, `idfn`
        = gt_frames - idtp, `idfp` = dt_frames - idtp; IDR = idtp / gt_frames,
        IDP = idtp / dt_frames, IDF1 = 2 idtp / (gt_frames + dt_frames), NaN where
        the denominator is 0.  The exact rules are in include/tao_amodal_hip.h,
        section "track-level identity".

        Returns {"columns": the names of cat_counts' columns, "cat_counts":
        int64[K, 6] = gt_tracks, gt_frames, dt_tracks, dt_frames, idtp, pairs
        with the category axis in the order of params.cat_ids, "idf1", "idp",
        "idr": float64[K], "total": {the six sums, "idfn", "idfp", "idf1", "idp",
        "idr"}, "frame_thr"}; with per_track=True "tracks": (ground-truth track
        ids, int64[n_gt, 3] = the assigned detection track's id or -1, the
        shared frames, the track's frames) and "dt_tracks": (detection track
        ids, int64[n_dt, 3] = the assigned ground-truth track's id or -1, kept,
        frames).  Every count is exact and the same from run to run; where
        several assignments reach the optimum, the one reported is one of them.

        `score_thr`: the operating point.  The tables hold every track up to the
        max_dets cut, whatever its score; with a threshold -- a float, or one per
        category in the order of params.cat_ids -- only the detection tracks
        whose score (the one Track-AP ranks them by) is >= it take part: whole
        tracks, never single boxes.  A NaN lets no track of its category pass,
        -inf every track.  None is the table as it is.  The result then holds
        "score_thr": float64[K] and is cached per threshold as well; the rule is
        in include/tao_amodal_hip.h, section "track-level score thresholds".
        tracking_curve() finds the threshold.
        Not available: iou_type="segm", use_cats = 0, multi-GPU runs."""
        return followers.identity(self, frame_thr, per_track, score_thr)

    def identity_lines(self, frame_thr=0.5, score_thr=None):
        """identity() as a small text table: the totals over the categories.
        Returned, not printed."""
        return followers.identity_lines(self.identity(frame_thr, score_thr=score_thr))

    def hota(self, alphas=None, frame_thr=0.5, per_frame=False, score_thr=None):
        """HOTA, DetA and AssA (Luiten et al., IJCV 2021; TrackEval's HOTA): the
        measure tracking papers print beside Track-AP and IDF1.  association()
        is a per-frame arg-max and identity() one assignment over whole tracks;
        HOTA makes a ONE-TO-ONE assignment in every frame, weighted by how well
        each pair of tracks aligns over the whole video, and scores every
        matched frame by the share of its two tracks' frames that are matched
        to each other.  Solved on the device on request (csrc/track_hota.hip).
        Callable after evaluate(), cached per (alphas, frame_thr).

        Rows are the tracks that survived the max_dets cut and the federated
        filter; a frame's candidates are the boxes of its video and category.
        The tracks that take part are identity(frame_thr)'s: ground-truth tracks
        marked "ignore" are left out, and so are the detection tracks it sets
        aside, so HOTA and IDF1 are computed over the same tracks.  `alphas`:
        the localisation thresholds, 1 to 32 strictly ascending values in (0, 1]
        (ValueError otherwise); None is TrackEval's np.arange(0.05, 0.99, 0.05).
        A matched frame counts at alpha where its box IoU >= alpha - eps.  The
        assignment is made once per frame, not once per alpha.  Every sum is
        carried as an integer in fixed point (2^30): the tables are exact and the
        same from run to run.  The exact rules are in include/tao_amodal_hip.h,
        section "track-level HOTA"; what differs from TrackEval's TAO
        preprocessing is in DESIGN.md section 8.

        Returns {"alphas", "frame_thr", "cat_counts": int64[K, 4] = gt_tracks,
        gt_frames, dt_tracks, dt_frames with the category axis in the order of
        params.cat_ids, the integers "tp", "fn", "fp", "loc": int64[K, A] and
        "ass": int64[K, A, 3] (loc and ass times 2^30), float64[K, A] "hota",
        "deta", "assa", "detre", "detpr", "assre", "asspr", "loca" with
        TrackEval's max(1, .) denominators (LocA is 1 without a match), NaN where
        the category has neither ground-truth nor detection frames, "total":
        the sums over the categories, their per-alpha ratios under the same
        names and the means over alpha "HOTA", "DetA", "AssA", "DetRe", "DetPr",
        "AssRe", "AssPr", "LocA" with "HOTA(0)", "LocA(0)", "HOTALocA(0)" at the
        first alpha (TrackEval's detection-averaged combination), "mean": those
        scalars averaged over the categories that have frames (its class-
        averaged combination)}; with per_frame=True "frames": per ground-truth
        frame (the ground-truth track id, the image id, the matched detection
        track's id or -1, its box IoU or 0).  `score_thr` as for identity(): the
        tracks that take part are identity(frame_thr, score_thr=score_thr)'s,
        and the result holds "score_thr".
        Not available: iou_type="segm", use_cats = 0, multi-GPU runs, the
        command line; recall per visibility window is clear()'s "vis_re" (the
        per-frame output here carries what a breakdown of DetRe needs)."""
        return followers.hota(self, alphas, frame_thr, per_frame, score_thr)

    def hota_lines(self, alphas=None, frame_thr=0.5, score_thr=None):
        """hota() as a small text table in per cent, in TrackEval's column order:
        the total and the class mean.  Returned, not printed."""
        return followers.hota_lines(self.hota(alphas, frame_thr, score_thr=score_thr))

    def clear(self, frame_thr=0.5, vis_rng=None, vis_lbl=None, per_track=False,
              per_frame=False, score_thr=None):
        """CLEAR MOT (Bernardin & Stiefelhagen, 2008; TrackEval's CLEAR): MOTA,
        MOTP, ID switches, fragmentations, mostly tracked / mostly lost -- the
        third of the measures printed beside Track-AP, with IDF1 (identity())
        and HOTA (hota()).  A ONE-TO-ONE assignment in every frame, as HOTA's,
        but each frame's weights depend on the frame before: the pair matched a
        step ago gets a bonus of 1000 over its box IoU, and an ID switch is
        scored against the ground truth's last match however long ago.  The
        frames of a (video, category) are a serial chain, walked on the device
        on request (csrc/track_clear.hip).  Callable after evaluate(), cached
        per (frame_thr, windows).

        Rows are the tracks that survived the max_dets cut and the federated
        filter.  The tracks that take part are identity(frame_thr)'s, as for
        hota(): MOTA, IDF1 and HOTA are computed over the same tracks and the
        same frame counts.  A pair is a candidate where its box IoU >=
        `frame_thr`; positions at which the cell has no ground-truth or no
        detection frame change no state.  `vis_rng`: up to 8 closed visibility
        windows (ValueError otherwise), by default association()'s, with
        `vis_lbl` their labels: how much of the recall and how many of the ID
        switches fall on occluded frames.  Every sum is an integer (MOTP's in
        fixed point, 2^30): the tables are exact and the same from run to run.
        The exact rules are in include/tao_amodal_hip.h, section "track-level
        CLEAR"; what differs from TrackEval is in DESIGN.md section 8.

        Returns {"frame_thr", "columns", "cat_counts": int64[K, 11] = gt_tracks,
        gt_frames, dt_tracks, dt_frames (identity()'s four), tp, idsw, frag, mt,
        pt, ml, motp_sum (times 2^30) with the category axis in the order of
        params.cat_ids, "fn", "fp": int64[K], float64[K] "mota" = (tp - fp - idsw)
        / max(1, tp + fn), "motp" = motp_sum / 2^30 / max(1, tp), "moda", "smota",
        "clr_re", "clr_pr", "clr_f1", "mtr", "ptr", "mlr" (over max(1,
        gt_tracks)), NaN where the category has neither ground-truth nor
        detection frames, "vis_counts": int64[n_vis, K, 4] = frames, matched,
        idsw, q_sum, "vis_rng", "vis_lbl", "vis_re": float64[n_vis, K] = matched /
        frames (NaN without frames), "total": the sums over the categories and
        the ratios of the sums, "mean": the ratios averaged over the categories
        that have frames}; with per_track=True "tracks": (the ground-truth track
        ids, int64[n_gt, 5] = present, matched, idsw, frag, 0 / 1 / 2 for mostly
        lost / partly / mostly tracked; zeros for an ignored track); with
        per_frame=True "frames": per ground-truth frame (the ground-truth track
        id, the image id, the matched detection track's id or -1, its box IoU
        or 0, the switch flag).  `score_thr` as for identity(): the tracks that
        take part are identity(frame_thr, score_thr=score_thr)'s, and the result
        holds "score_thr".
        Not available: iou_type="segm", use_cats = 0, multi-GPU runs, the
        command line; FP per frame (no table holds a video's frame count)."""
        return followers.clear(self, frame_thr, vis_rng, vis_lbl, per_track, per_frame,
                               score_thr)

    def clear_lines(self, frame_thr=0.5, vis_rng=None, vis_lbl=None, score_thr=None):
        """clear() as a small text table in per cent, in TrackEval's CLEAR column
        order: the total and the class mean, then a line per visibility window
        with CLR_Re and IDSW.  Returned, not printed."""
        return followers.clear_lines(self.clear(frame_thr, vis_rng, vis_lbl,
                                                score_thr=score_thr))

    def tracking_curve(self, score_thrs=None, frame_thr=0.5, alphas=None,
                       measures=("identity", "hota", "clear")):
        """identity(), hota() and clear() at a list of score thresholds: at
        which score is IDF1, HOTA or MOTA best?  None of them is monotone in the
        threshold.  `score_thrs`: 1 to 64 strictly ascending doubles (ValueError
        otherwise), each applied to every category; None takes the distinct
        values of the 0 %, 10 %, ... 90 % quantiles (scores that occur) of the
        finite scores of the table's detection tracks, so that the first row is
        the table without a threshold whenever no score is a NaN.  The frames'
        shares are counted once and the identity's assignment is solved for all
        thresholds in one launch; HOTA and CLEAR run once per threshold.
        `measures`: which of "identity", "hota", "clear" (the identity's counts
        are formed in any case: the other two are computed over its tracks).
        Callable after evaluate(); not cached.

        Returns {"score_thrs": float64[T], "cat_counts": int64[T, K, 6], the
        identity's, the category axis in the order of params.cat_ids, float64[T,
        K] "idf1", "hota", "deta", "assa" (the means over alpha), "mota", "motp"
        and int64[T, K] "idsw", NaN where the category has no frames, "total":
        the [T] arrays of what identity()'s, hota()'s and clear()'s "total" hold
        as one number each -- the counts (gt_tracks .. dt_frames, idtp, tp, idsw,
        ...), "idf1", "idp", "idr", "HOTA", "DetA", "AssA", ..., "mota", "motp",
        ... --, "mean": hota()'s and clear()'s class means alike, "best": for
        "IDF1", "HOTA" and "MOTA" {"index", "score_thr", "value"} of the greatest
        total (the lowest threshold among equal ones; NaN rows are skipped),
        "best_per_category": for the same names float64[K], the maximising
        threshold per category (NaN without frames), which can be passed back as
        `score_thr`, "frame_thr", "alphas", "measures"}.  Row t holds exactly
        the numbers of the single calls with score_thr=score_thrs[t].
        Not available: iou_type="segm", use_cats = 0, multi-GPU runs."""
        return followers.tracking_curve(self, score_thrs, frame_thr, alphas, measures)

    def curve_lines(self, c):
        """tracking_curve()'s result `c` as a small text table: a line per
        threshold with dt_tracks, IDF1, HOTA, DetA, AssA, MOTA in per cent and
        IDSW.  Returned, not printed."""
        return followers.curve_lines(c)

    def impact_lines(self, iou_thr=0.5, bg_thr=0.1):
        """error_impact() as a small text table: a line per (area, time) range,
        AP and the dAP of the eight fixes.  Returned, not printed."""
        return _core.impact_lines(self, iou_thr, bg_thr)

    def confusion(self, iou_thr=0.5, bg_thr=0.1):
        """Which category each CLS and BOTH detection track of
        error_types(iou_thr, bg_thr) was taken for, per (area, time) range:
        LVISEval.confusion() rule for rule on tracks.  For every (range,
        predicted category, ground-truth category) with at least one such
        track: `cls`, `both`, `unheld` (CLS tracks on a ground-truth track that
        is missed) and `adopted` (the track error_impact()'s CLS fix hands to
        that ground-truth track).  Computed on the device on request
        (csrc/confusion.hip, the kernels of the image level) from the links of
        the track-level breakdown, as a sparse table.  Callable after
        evaluate(), cached per (iou_thr, bg_thr).  The exact rules are in
        include/tao_amodal_hip.h, section "confusion".

        Returns {"columns": ["cls", "both", "unheld", "adopted"], "rng_lbl":
        the (area label, time label) of every range, "rng": int32[n] the range
        index (area x durations flattened, as in error_types()), "dt_cat",
        "gt_cat": int64[n] category ids, "counts": int64[n, 4]}, sorted by
        (range, place of dt_cat in params.cat_ids, place of gt_cat); with a
        params.cat_ids subset only pairs of those categories.  Not available
        where error_types() is not."""
        return _core.confusion(self, iou_thr, bg_thr)

    def confusion_matrix(self, iou_thr=0.5, bg_thr=0.1, rng=0, column="cls"):
        """One column of confusion() for the range of index `rng` as a dense
        int64[K, K] in the order of params.cat_ids, rows the predicted
        category; scattered on the host.  The diagonal is zero."""
        return _core.confusion_matrix(self, iou_thr, bg_thr, rng, column)

    def confusion_lines(self, iou_thr=0.5, bg_thr=0.1, rng=0, top=10):
        """confusion() as a small text table: the `top` pairs of the range of
        index `rng`, most `adopted` first, then most `cls`, then by (dt_cat,
        gt_cat); both ids with the annotation file's category names (the id
        again where a category has none) and the four counts.  Returned, not
        printed."""
        return _core.confusion_lines(self, iou_thr, bg_thr, rng, top)

    def _summarize(self, summary_type, iou_thr=None, area_rng="all",
                   time_rng="all", freq_group_idx=None):
        aidx = [i for i, lbl in enumerate(self.params.area_rng_lbl)
                if lbl == area_rng]
        tidx_ = [i for i, lbl in enumerate(self.params.time_rng_lbl)
                 if lbl == time_rng]
        if summary_type == "ap":
            s = self.eval["precision"]
            if iou_thr is not None:
                s = s[np.where(iou_thr == self.params.iou_thrs)[0]]
            s = s[:, :, :, aidx, tidx_]
        else:
            s = self.eval["recall"]
            if iou_thr is not None:
                s = s[np.where(iou_thr == self.params.iou_thrs)[0]]
            s = s[:, :, aidx, tidx_]
        return masked_mean(s)

    def summarize(self):
        if not self.eval:
            raise RuntimeError("Please run accumulate() first.")
        max_dets = self.params.max_dets
        S = self._summarize
        hp = "highly-and-partially-occluded"
        jobs = [("AP", lambda: S("ap")),
                ("AP50", lambda: S("ap", iou_thr=0.50)),
                ("AP75", lambda: S("ap", iou_thr=0.75)),
                ("AP-HP", lambda: S("ap", area_rng=hp)),
                ("AP50-HP", lambda: S("ap", area_rng=hp, iou_thr=0.50)),
                ("AP75-HP", lambda: S("ap", area_rng=hp, iou_thr=0.75))]
        for rng in ["small", "medium", "large"]:
            jobs.append((("AP", "area", rng, max_dets), lambda rng=rng: S("ap", area_rng=rng)))
        for rng in ["short", "medium", "long"]:
            jobs.append((("AP", "time", rng, max_dets), lambda rng=rng: S("ap", time_rng=rng)))
        jobs.append(("AR@{}".format(max_dets), lambda: S("ar")))
        for rng in ["small", "medium", "large"]:
            jobs.append((("AR", "area", rng, max_dets), lambda rng=rng: S("ar", area_rng=rng)))
        for rng in ["short", "medium", "long"]:
            jobs.append((("AR", "time", rng, max_dets), lambda rng=rng: S("ar", time_rng=rng)))
        for key, value in summaries(jobs):
            self.results[key] = value

    def run(self, show_progress=False):
        self.evaluate(show_progress=show_progress)
        self.accumulate()
        with timed("summarize"):
            self.summarize()

    def result_lines(self):
        template = (" {:<18} {} @[ IoU={:<9} | area={:>6s} | dur={:>6s} | "
                    "maxDets={:>3d} catIds={:>3s}] = {:0.3f}")
        lines = []
        for key, value in self.results.items():
            max_dets = self.params.max_dets
            is_ap = "AP" in key
            area = time = "all"
            if isinstance(key, tuple):
                kind, rng, max_dets = key[1:]
                if kind == "time":
                    time = rng[0]
                elif kind == "area":
                    area = rng[0]
                else:
                    raise ValueError("This should not happen")
            if len(key) > 2 and key[2].isdigit():
                iou = "{:0.2f}".format(float(key[2:4]) / 100)
            else:
                iou = "{:0.2f}:{:0.2f}".format(self.params.iou_thrs[0],
                                               self.params.iou_thrs[-1])
            group = key[2] if len(key) > 2 and key[2] in ["r", "c", "f"] else "all"
            lines.append(template.format(
                "Average Precision" if is_ap else "Average Recall",
                "(AP)" if is_ap else "(AR)", iou, area, time, max_dets, group,
                value))
        return lines

    def print_results(self):
        for line in self.result_lines():
            self.logger.info(line)

    def get_results(self):
        if not self.results:
            self.logger.warning("results is empty. Call run().")
        return self.results
