"""Shared machinery of the two evaluator classes: running a flattened problem
on the GPU, the numpy-side summaries (kept in numpy so that the means are
computed by the very same pairwise summation as the reference), and the lazy
views that expose the reference's bulky per-cell state (``ious``,
``eval_imgs`` / ``eval_vids``, ``dt_pointers``) without materialising it.
"""
import datetime
from collections.abc import Mapping, Sequence

import numpy as np

N_THR, N_REC = 10, 101


def masked_mean(s):
    """``np.mean(s[s > -1])`` or -1 (reference lvis_amodal/eval.py:453-457,
    tao_amodal/eval.py:619-623)."""
    sel = s[s > -1]
    if len(sel) == 0:
        return -1
    return np.mean(sel)


def summaries(jobs):
    """``[(key, thunk), ...]`` -> yields ``(key, thunk())`` in the order given:
    the masked means of a summary are independent of each other and numpy's
    slicing, comparing and adding run without the interpreter lock, so they go
    to a few threads (46 means over 58 + 194 MB of tables: 0.08 s one after the
    other).  The caller fills its result dict as the pairs arrive -- the
    reference's order of insertion, a key written twice keeping the LAST value
    (lvis_amodal/eval.py:497-499) -- and a thunk that raises (edited params:
    fewer ranges than the labels name) raises HERE, at its place in the order,
    behind the results before it, like the reference's loop."""
    if len(jobs) < 4:
        for k, f in jobs:
            yield k, f()
        return
    from concurrent.futures import ThreadPoolExecutor
    pool = ThreadPoolExecutor(max_workers=4)
    try:
        futures = [pool.submit(f) for _, f in jobs]
        for (k, _), fu in zip(jobs, futures):
            yield k, fu.result()
    finally:
        pool.shutdown(wait=True, cancel_futures=True)


TIMING = {}   # wall-clock seconds per stage, filled when TAOAMD_TIMING is set


import threading as _threading
_TIMING_LOCK = _threading.Lock()


def timed(name):
    """Context manager adding the elapsed wall-clock to TIMING[name]."""
    import contextlib
    import os
    import time

    @contextlib.contextmanager
    def cm():
        if not os.environ.get("TAOAMD_TIMING"):
            yield
            return
        t0 = time.perf_counter()
        try:
            yield
        finally:
            with _TIMING_LOCK:      # (the CLI's two levels time the same keys)
                TIMING[name] = TIMING.get(name, 0.0) + time.perf_counter() - t0
    return cm()


class GpuRun:
    """One evaluator pass on the device, split like the reference's API:
    evaluate() = ranges + sort + [track IoU] + match, accumulate() = sweep."""

    def __init__(self, flat, device=None, iou_3d_type="3d_iou", constants=None):
        """``constants`` (EvalConstants): edited ``params`` thresholds / ranges;
        None = the reference's defaults."""
        import torch
        from .. import engine
        self.constants = constants if constants is not None and not constants.default \
            else None
        if not torch.cuda.is_available():
            raise RuntimeError(
                "tao_amodal_amd evaluates on an AMD GPU through its HIP "
                "extension; no GPU is visible and there is no CPU fallback.")
        self.engine = engine
        self.torch = torch
        self.flat = flat
        self.iou_3d_type = iou_3d_type
        self.device = torch.device(device or "cuda")
        with timed("upload+plan"):
            self.dp = engine.DeviceProblem(flat, self.device, iou_3d_type)
            self.ws = engine.Workspace(self.dp)
            torch.cuda.synchronize(self.device)
        self._detail = None
        self._head_done = False      # sort + IoU matrix of this problem are in the workspace
        self._error_pass = False     # error_table() ran the pass evaluate() left out
        self.near_threshold_pairs = 0
        self.precision = self.recall = None

    def evaluate(self):
        e = self.engine
        c = self.constants
        if c is not None and not c.single:
            return         # several blocks of thresholds: every pass in accumulate()
        with timed("kernels"), applied(c):
            # (frame-order guard of the 3D IoU applied before the match, on
            # the device: engine.stage_iou_guard; its count is read later)
            e.run_guarded(self.dp, self.ws, self.flat, upto="match",
                          read_count=False)
            self._head_done = True
            import os
            if os.environ.get("TAOAMD_TIMING"):
                self.torch.cuda.synchronize(self.device)

    def accumulate(self):
        c = self.constants
        if c is not None:
            return self._accumulate_blocks(c)
        with timed("kernels"):
            self.engine.stage_accumulate(self.dp, self.ws)
            self.torch.cuda.synchronize(self.device)
            self.near_threshold_pairs = self.engine.guarded_pairs(self.dp, self.ws)
        with timed("download"):
            self.precision = self.ws.precision.cpu().numpy()
            self.recall = self.ws.recall.cpu().numpy()

    def _accumulate_blocks(self, c):
        """Edited constants: the kernels take N_THR IoU thresholds, N_REC
        recall thresholds and their own number of ranges per pass -- the
        caller's arrays are cut into such blocks (EvalConstants) and every
        block's slice of the tables is put where the caller's order has it.
        IoU thresholds are independent of each other (L/eval.py:234-277), recall
        thresholds (:406-410) and ranges (:140-145, T/eval.py:271-276) too."""
        e, dp, ws = self.engine, self.dp, self.ws
        K = dp.n_cat
        self.precision = np.empty((c.T, c.R, K, c.n_rng))
        self.recall = np.empty((c.T, K, c.n_rng))
        first = True
        for bi, (t_idx, t_val) in enumerate(c.thr_blocks):
            for bk, (_, slots) in enumerate(c.rng_blocks):
                ks = np.array([k for k, _ in slots], dtype=np.int64)
                out = np.array([i for _, i in slots], dtype=np.int64)
                for bj, (r_idx, r_val) in enumerate(c.rec_blocks):
                    with timed("kernels"), applied(c, bi, bj, bk):
                        if bj == 0 and not (c.single and first):
                            # (the sort and the IoU matrix once: they depend on
                            # neither thresholds nor ranges -- ADVICE r5)
                            e.run_guarded(dp, ws, self.flat, upto="match", read_count=False,
                                          head=not self._head_done)
                            self._head_done = True
                        first = False
                        e.stage_accumulate(dp, ws)
                        self.torch.cuda.synchronize(self.device)
                        # (per block, under the block's constants: an unprepared
                        # pass clears the flag of the pass before it)
                        e.sweep_ok(dp, ws)
                    with timed("download"):
                        p = ws.precision[:len(t_idx), :len(r_idx)].cpu().numpy()
                        self.precision[np.ix_(t_idx, r_idx, np.arange(K), out)] = p[..., ks]
                        if bj == 0:
                            rc = ws.recall[:len(t_idx)].cpu().numpy()
                            self.recall[np.ix_(t_idx, np.arange(K), out)] = rc[..., ks]
        self.near_threshold_pairs = e.guarded_pairs(dp, ws)
        if not c.rec_sorted:
            # the reference fills a row's recall thresholds IN THE CALLER'S
            # ORDER and stops at the first one the category never reaches (the
            # bare `except` of L/eval.py:406-410): what follows stays 0
            never = np.maximum.accumulate(self.precision == 0, axis=1)
            self.precision[never] = 0

    # ------------------------------------------------------ lazy detail
    def detail(self):
        """Per-detection match indices / IoUs (a second, detail-mode pass,
        only when the per-cell views are actually inspected)."""
        if self._detail is None:
            c = self.constants
            if c is not None and not c.single:
                raise NotImplementedError(
                    "the per-cell views (ious, eval_imgs / eval_vids, dt_pointers) "
                    "are kept for up to %d IoU thresholds and the reference's "
                    "number of ranges" % N_THR)
            with applied(c):
                self._detail = self.engine.evaluate_flat(
                    self.flat, self.device, detail=True,
                    iou_3d_type=self.iou_3d_type)
        return self._detail

    def thr_slots(self, views=True):
        """Place of the caller's i-th IoU threshold among the kernels' combos
        (`views`: for the per-cell views, which also want the caller's ranges
        slot for slot)."""
        c = self.constants
        if c is None:
            return list(range(N_THR))
        if views and not c.single:
            self.detail()        # raises
        slot = np.empty(c.T, dtype=np.int64)
        slot[c.thr_blocks[0][0]] = np.arange(c.T)
        return slot.tolist()

    def score_table(self):
        """eval["scores"][T, R, K, n_rng] in the caller's order of thresholds:
        the score of the detection at which recall first reaches each recall
        threshold (pycocotools' ss[ri] = dtScoresSorted[pi]; the index is the
        reference's rec_thrs_insert_idx, L/eval.py:406-417), from the rows the
        workspace holds after accumulate() (engine.stage_scores)."""
        if self.precision is None:
            raise RuntimeError("Please run accumulate() first.")
        c = self.constants
        if c is not None and not c.single:
            raise NotImplementedError(
                "eval['scores'] is kept for up to %d IoU thresholds, %d recall "
                "thresholds and the reference's number of ranges" % (N_THR, N_REC))
        with timed("kernels"), applied(c):
            self.engine.stage_scores(self.dp, self.ws)
            self.torch.cuda.synchronize(self.device)
        with timed("download"):
            s = self.ws.scores.cpu().numpy()
        if c is None:
            return s
        r_idx = c.rec_blocks[0][0]
        out = np.empty((c.T, c.R) + s.shape[2:])
        out[:, r_idx] = s[self.thr_slots(), :c.R]
        if not c.rec_sorted:
            # the reference fills a row IN THE CALLER'S ORDER and stops at the
            # first threshold the category never reaches (the bare `except` of
            # L/eval.py:412-416): what follows stays 0.  Never reached: above
            # the category's recall, or a category without detections.
            rec = np.empty(c.R)
            rec[r_idx] = c.rec_blocks[0][1][:c.R]
            no_rows = np.diff(np.asarray(self.dp.cat_off_host)) == 0
            unreached = (rec[None, :, None, None] > self.recall[:, None]) \
                | no_rows[None, None, :, None]
            never = np.maximum.accumulate(unreached, axis=1)
            out[never & (self.recall[:, None] != -1)] = 0
        return out

    def error_table(self, thr_index, bg_thr, per_detection=False):
        """(dt_counts[n_rng, K, 7], gt_counts[n_rng, K, 3], dt_type[n_dt, n_rng]
        or None) at the caller's `thr_index`-th IoU threshold, ranges in the
        caller's order (engine.stage_error_types at the image level,
        engine.stage_track_error_types at the track level; the definitions are
        in include/tao_amodal_hip.h), from the pass the workspace holds after
        evaluate()."""
        track = self.flat.kind == "tao"
        c, slot = self._error_pass_at(thr_index)
        e = self.engine
        with timed("kernels"), applied(c):
            stage = e.stage_track_error_types if track else e.stage_error_types
            stage(self.dp, self.ws, slot, bg_thr, per_detection)
            self.torch.cuda.synchronize(self.device)
        with timed("download"):
            dt_counts = self.ws.err_dt_counts.cpu().numpy()
            gt_counts = self.ws.err_gt_counts.cpu().numpy()
            dt_type = self.ws.err_dt_type[:self.dp.n_dt].cpu().numpy() if per_detection \
                else None
        if c is not None:
            # kernel range slot -> the caller's range
            ks = self._range_slots(c)
            dt_counts, gt_counts = dt_counts[ks], gt_counts[ks]
            if dt_type is not None:
                dt_type = np.ascontiguousarray(dt_type[:, ks])
        return dt_counts, gt_counts, dt_type

    @staticmethod
    def _range_slots(c):
        return [k for k, _ in sorted(c.rng_blocks[0][1], key=lambda ki: ki[1])]

    def _error_pass_at(self, thr_index):
        """What error_table(), impact_table() and confusion_table() share: the
        refusals, the kernels' slot of the caller's threshold, and the match
        pass where evaluate() left it out.  Returns (constants, slot)."""
        c = self.constants
        track = self.flat.kind == "tao"
        if track and self.iou_3d_type != "3d_iou":
            raise NotImplementedError(
                "error_types() with iou_3d_type=%r: defined for '3d_iou'" % self.iou_3d_type)
        if self.dp.mask_iou:
            raise NotImplementedError("error_types() with iou_type='segm': boxes only")
        if not self.flat.get("use_cats", True):
            raise NotImplementedError(
                "error_types() with use_cats = 0: one pooled category has no class confusion")
        if c is not None and (len(c.thr_blocks) > 1 or len(c.rng_blocks) > 1):
            raise NotImplementedError(
                "error_types() is kept for up to %d IoU thresholds and one block of "
                "ranges" % N_THR)
        slot = self.thr_slots(views=False)[thr_index]
        e = self.engine
        with timed("kernels"), applied(c):
            if c is not None and not c.single and not self._error_pass:
                # one block of thresholds and of ranges, yet not the kernels'
                # tables slot for slot: evaluate() left the pass to accumulate(),
                # whose blocks repeat this very match
                e.run_guarded(self.dp, self.ws, self.flat, upto="match", read_count=False,
                              head=not self._head_done,
                              match_gt=e.error_match_gt(self.dp, self.ws))
                self._head_done = self._error_pass = True
        return c, slot

    def impact_table(self, thr_index, bg_thr):
        """(precision[9, R, K, n_rng], num_gt[9, K, n_rng]) of the nine fixes at
        the caller's `thr_index`-th IoU threshold: recall thresholds and ranges
        in the caller's order (engine.stage_error_impact at the image level,
        engine.stage_track_error_impact at the track level; the definition is
        in include/tao_amodal_hip.h), from the pass the workspace holds after
        evaluate().  Refuses what error_table() refuses, in its words."""
        track = self.flat.kind == "tao"
        c = self.constants
        if c is not None and len(c.thr_blocks) == 1 and len(c.rng_blocks) == 1 \
                and len(c.rec_blocks) > 1:
            raise NotImplementedError(
                "error_impact() is kept for up to %d recall thresholds" % N_REC)
        c, slot = self._error_pass_at(thr_index)
        with timed("kernels"), applied(c):
            e = self.engine
            stage = e.stage_track_error_impact if track else e.stage_error_impact
            stage(self.dp, self.ws, slot, bg_thr)
            self.torch.cuda.synchronize(self.device)
        with timed("download"):
            p = self.ws.imp_precision.cpu().numpy()
            num_gt = self.ws.imp_num_gt.cpu().numpy().astype(np.int64)
        if c is None:
            return p, num_gt
        ks = self._range_slots(c)
        r_idx = c.rec_blocks[0][0]
        out = np.empty((p.shape[0], c.R) + p.shape[2:3] + (len(ks),))
        out[:, r_idx] = p[:, :c.R][..., ks]
        if not c.rec_sorted:
            # the reference fills a row IN THE CALLER'S ORDER and stops at the
            # first threshold the category never reaches (see accumulate)
            out[np.maximum.accumulate(out == 0, axis=1)] = 0
        return out, num_gt[..., ks]

    def confusion_table(self, thr_index, bg_thr):
        """(rng int32[n], dt_cat int64[n], gt_cat int64[n], counts int64[n, 4],
        K): the category pairs the CLS and BOTH rows confuse at the caller's
        `thr_index`-th IoU threshold (engine.stage_confusion; the definition is
        in include/tao_amodal_hip.h): the caller's range index, the two
        categories as indices into the tables' K categories and (cls, both,
        unheld, adopted), sorted by (range, dt_cat, gt_cat), from the pass the
        workspace holds after evaluate().  Refuses what error_table() refuses,
        in its words."""
        c, slot = self._error_pass_at(thr_index)
        with timed("kernels"), applied(c):
            self.engine.stage_confusion(self.dp, self.ws, slot, bg_thr)
            self.torch.cuda.synchronize(self.device)
        with timed("download"):
            ws, n = self.ws, self.ws.conf_n
            off = ws.conf_off.cpu().numpy()
            gt_cat = ws.conf_gt_cat[:n].cpu().numpy().astype(np.int64)
            counts = ws.conf_counts[:n].cpu().numpy().astype(np.int64)
        K = self.dp.n_cat
        row = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
        rng, dt_cat = row // K, row % K
        if c is not None:
            # kernel range slot -> the caller's range; the slots it has no range for go
            to = np.full((len(off) - 1) // K, -1, dtype=np.int64)
            ks = self._range_slots(c)
            to[ks] = np.arange(len(ks))
            rng = to[rng]
            keep = np.flatnonzero(rng >= 0)
            keep = keep[np.argsort(rng[keep], kind="stable")]
            rng, dt_cat, gt_cat, counts = rng[keep], dt_cat[keep], gt_cat[keep], counts[keep]
        return rng.astype(np.int32), dt_cat, gt_cat, counts, K

    def _followers_at(self, what, ann_vis):
        """What association_table(), occlusion_table(), identity_table() and
        hota_table() share: the refusals, in the name `what` of the caller's method, and
        (`ann_vis` not None) the frames' own visibility, gathered from the
        annotations' column and uploaded on the first call."""
        if self.flat.kind != "tao":
            raise NotImplementedError(what + " is the track level's")
        if self.dp.mask_iou:
            raise NotImplementedError(what + " with iou_type='segm': boxes only")
        if not self.flat.get("use_cats", True):
            raise NotImplementedError(
                what + " with use_cats = 0: the candidates of a ground-truth track "
                "are the detection tracks of its category")
        if ann_vis is not None and self.dp.t.get("gt_frame_vis") is None:
            with timed("upload+plan"):
                rows = self.flat.gt_frame_box.index
                self.engine.set_frame_visibility(
                    self.dp, np.asarray(ann_vis, dtype=np.float64)[rows])

    def association_table(self, frame_thr, vis_rng, ann_vis):
        """The per-frame followers of the ground-truth tracks
        (engine.stage_track_association; the definition is in
        include/tao_amodal_hip.h) at the per-frame threshold `frame_thr` and the
        visibility windows `vis_rng`: dict(gt_assoc int32[n_gt, 7] with the
        primary as a table row, cat_counts int64[K, 8], vis_counts int64[n_vis,
        K, 3], best int32[n_gt_frames] as in-cell indices, best_iou).  `ann_vis`:
        the `visibility` column of the ground-truth annotations the tables were
        built from; the frames' own is gathered and uploaded on the first call.
        Reads the track tables alone: no constants, no match, no IoU matrix."""
        self._followers_at("association()", ann_vis)
        e, dp, ws = self.engine, self.dp, self.ws
        with timed("kernels"):
            e.stage_track_association(dp, ws, frame_thr, vis_rng)
            self.torch.cuda.synchronize(self.device)
        with timed("download"):
            n_gf = int(dp.t["gt_frame_pos"].numel())
            return self._download(
                gt_assoc=(ws.assoc_gt, dp.n_gt), cat_counts=ws.assoc_cat_counts,
                vis_counts=(ws.assoc_vis_counts, (0, dp.n_cat, 3)),
                best=(ws.assoc_best, n_gf), best_iou=(ws.assoc_best_iou, n_gf))

    def occlusion_table(self, frame_thr, vis_rng, recover, len_edges, ann_vis):
        """Whether the follower of a ground-truth track is kept through occlusion
        (engine.stage_track_occlusion; the definition is in
        include/tao_amodal_hip.h): the runs of frames whose visibility lies in
        the closed window `vis_rng` = (lo, hi), over the followers at `frame_thr`:
        dict(gt_occ int32[n_gt, 4], counts int64[K, n_len, 11], episodes
        int32[n_ep, 9] with entry and after as in-cell indices).  `ann_vis` as for
        association_table(); refuses what it refuses."""
        self._followers_at("occlusions()", ann_vis)
        dp, ws = self.dp, self.ws
        with timed("kernels"):
            self.engine.stage_track_occlusion(dp, ws, frame_thr, vis_rng[0], vis_rng[1], recover,
                                              len_edges, episodes=True)
            self.torch.cuda.synchronize(self.device)
        with timed("download"):
            return self._download(gt_occ=(ws.occ_gt, dp.n_gt), counts=ws.occ_counts,
                                  episodes=(ws.occ_episodes, ws.occ_n))

    @staticmethod
    def _download(**tables):
        """Device tables on the host: name=tensor (all of it), name=(tensor, n)
        (its first n rows) or name=(tensor or None, shape) (for None the int64
        zeros of `shape`: a table of no windows)."""
        out = {}
        for name, table in tables.items():
            t, n = table if isinstance(table, tuple) else (table, None)
            if t is None:
                out[name] = np.zeros(n, dtype=np.int64)
            else:
                out[name] = (t if n is None or isinstance(n, tuple) else t[:n]).cpu().numpy()
        return out

    def _kept(self, frame_thr, score_thr, per_track=False, rerun=False):
        """(keep uint8[T, n_dt], cat_counts int64[T, K, 6]) on the device: the
        identity's kept column and counts at `frame_thr`, a row per layer --
        what hota_table(), clear_table() and curve_tables() run over.
        `score_thr` None: the one row of the unthresholded identity (views of
        ws.ident_keep and ws.ident_cat_counts), reused where the workspace holds
        it for `frame_thr` unless `rerun`.  float64[K]: a threshold per category
        in the tables' order, one layer; float64[T, K]: a table of layers
        (engine.stage_track_identity_at, in one launch; `per_track` as there)."""
        e, dp, ws = self.engine, self.dp, self.ws
        if score_thr is None:
            if rerun:
                e.stage_track_identity(dp, ws, frame_thr)
            keep = e.kept_tracks(dp, ws, float(frame_thr), None)
            return keep[None], ws.ident_cat_counts[None]
        thr = np.ascontiguousarray(score_thr, dtype=np.float64)
        if thr.ndim < 2:
            thr = thr.reshape(1, -1)
            if thr.shape[1] != dp.n_cat:
                raise ValueError("score_thr: %d thresholds for the tables' %d categories"
                                 % (thr.shape[1], dp.n_cat))
        e.stage_track_identity_at(dp, ws, frame_thr, thr, per_track=per_track)
        return ws.at_keep, ws.at_cat_counts

    def identity_table(self, frame_thr, score_thr=None):
        """The identity measures' tables (engine.stage_track_identity; the
        definition is in include/tao_amodal_hip.h) at the per-frame threshold
        `frame_thr`: dict(cat_counts int64[K, 6], gt_ident int32[n_gt, 2],
        dt_ident int32[n_dt, 2], rows as table rows).  With `score_thr`
        (float64[K] in the tables' category order) over the detection tracks at
        or above it (engine.stage_track_identity_at; section "track-level score
        thresholds").  Reads the track tables alone; refuses what
        association_table() refuses."""
        self._followers_at("identity()", None)
        dp, ws = self.dp, self.ws
        with timed("kernels"):
            _, counts = self._kept(frame_thr, score_thr, per_track=True, rerun=True)
            gt, dt = (ws.ident_gt, ws.ident_dt) if score_thr is None else (ws.at_gt[0], ws.at_dt[0])
            self.torch.cuda.synchronize(self.device)
        with timed("download"):
            return self._download(cat_counts=counts[0], gt_ident=(gt, dp.n_gt),
                                  dt_ident=(dt, dp.n_dt))

    def hota_table(self, alphas, frame_thr, score_thr=None):
        """HOTA's integer tables (engine.stage_track_hota; the definition is in
        include/tao_amodal_hip.h) at the localisation thresholds `alphas` (eps
        already subtracted) over the tracks identity_table(frame_thr, score_thr)
        keeps: dict(cat_counts int64[K, 6] of that identity, tp and loc int64[K,
        A], ass int64[K, A, 3], match int32[n_gt_frames] as in-cell indices,
        match_iou).  Reads the track tables alone; refuses what identity_table()
        refuses."""
        self._followers_at("hota()", None)
        dp, ws, e = self.dp, self.ws, self.engine
        with timed("kernels"):
            keep, counts = self._kept(frame_thr, score_thr)
            e.stage_track_hota(dp, ws, alphas, frame_thr, keep=keep[0])
            self.torch.cuda.synchronize(self.device)
        with timed("download"):
            n_gf = int(dp.t["gt_frame_pos"].numel())
            return self._download(cat_counts=counts[0], tp=ws.hota_tp, loc=ws.hota_loc,
                                  ass=ws.hota_ass, match=(ws.hota_match, n_gf),
                                  match_iou=(ws.hota_match_iou, n_gf))

    def clear_table(self, frame_thr, vis_rng, ann_vis, score_thr=None):
        """CLEAR MOT's integer tables (engine.stage_track_clear; the definition is
        in include/tao_amodal_hip.h) at the per-frame threshold `frame_thr` and the
        visibility windows `vis_rng`, over the tracks identity_table(frame_thr,
        score_thr) keeps: dict(ident_counts int64[K, 6] of that identity,
        cat_counts int64[K, 7], vis_counts int64[n_vis, K, 4], gt_clear
        int32[n_gt, 4], match int32[n_gt_frames] as in-cell indices, match_iou, sw
        uint8).  `ann_vis` as for association_table(); refuses what it refuses."""
        self._followers_at("clear()", ann_vis)
        dp, ws, e = self.dp, self.ws, self.engine
        with timed("kernels"):
            keep, counts = self._kept(frame_thr, score_thr)
            e.stage_track_clear(dp, ws, frame_thr, vis_rng, keep=keep[0])
            self.torch.cuda.synchronize(self.device)
        with timed("download"):
            n_gf = int(dp.t["gt_frame_pos"].numel())
            return self._download(
                ident_counts=counts[0], cat_counts=ws.clear_cat_counts,
                vis_counts=(ws.clear_vis_counts, (0, dp.n_cat, 4)), gt_clear=(ws.clear_gt, dp.n_gt),
                match=(ws.clear_match, n_gf), match_iou=(ws.clear_match_iou, n_gf),
                sw=(ws.clear_sw, n_gf))

    def curve_tables(self, frame_thr, thr_tables, alphas, measures):
        """The integer tables of tracking_curve(): the identity over every layer
        of `thr_tables` float64[T, K] (the tables' category order) in one launch
        (engine.stage_track_identity_at), then -- for "hota" and "clear" in
        `measures` -- a host loop of engine.stage_track_hota / stage_track_clear
        over the layers' kept columns.  dict(cat_counts int64[T, K, 6], tp and loc
        int64[T, K, A], ass int64[T, K, A, 3], clear int64[T, K, 7]; what was not
        asked for is absent).  Refuses what identity_table() refuses."""
        self._followers_at("tracking_curve()", None)
        dp, ws, e = self.dp, self.ws, self.engine
        out = {}
        with timed("kernels"):
            keep, counts = self._kept(frame_thr, thr_tables)
            out["cat_counts"] = counts.cpu().numpy()
            rows = {k: [] for k in ("tp", "loc", "ass", "clear")}
            for t in range(len(keep)):
                if "hota" in measures:
                    e.stage_track_hota(dp, ws, alphas, frame_thr, keep=keep[t])
                    for k, v in (("tp", ws.hota_tp), ("loc", ws.hota_loc), ("ass", ws.hota_ass)):
                        rows[k].append(v.cpu().numpy())
                if "clear" in measures:
                    e.stage_track_clear(dp, ws, frame_thr, [], keep=keep[t])
                    rows["clear"].append(ws.clear_cat_counts.cpu().numpy())
        out.update({k: np.stack(v) for k, v in rows.items() if v})
        return out

    def pointer_tables(self):
        """What eval['dt_pointers'] is read from: the detections' ids and
        (matched, ignored) words in the sweep's order (category-major, stable
        descending score), num_gt and the categories' row offsets."""
        n = self.dp.n_dt
        ws = self.ws
        order = ws.order[:n].cpu().numpy().astype(np.int64)
        return {"ids": np.asarray(self.flat.dt_id)[order],
                "matched": ws.matched[:n].cpu().numpy().view(np.uint64),
                "ignored": ws.ignored[:n].cpu().numpy().view(np.uint64),
                "num_gt": ws.num_gt.cpu().numpy(),
                "cat_off": np.asarray(self.dp.cat_off_host, dtype=np.int64)}


def _bit(words, combo):
    return ((words[..., combo // 64] >> np.uint64(combo % 64))
            & np.uint64(1)).astype(bool)


def restrict_to_params(gt, dt, unit, unit_ids, cat_ids, use_cats):
    """The reference's ``_prepare`` (lvis_amodal/eval.py:59-105,
    tao_amodal/eval.py:178-233) for edited ``params``: the ground truth and the
    predictions of the images / videos in ``unit_ids`` only.  ``unit`` is
    "image" or "video"; ``cat_ids`` = params.cat_ids in the caller's order.
    Returns (gt columns, dt columns, cat_pos): cat_pos[i] = index of
    cat_ids[i] in the sorted category table -- the category axis of the result
    tables is taken through it (categories are independent of each other when
    use_cats = 1, so a category subset is a selection of result columns; the
    class-agnostic pool of use_cats = 0 is formed from all categories and a
    subset there raises).  Unknown ids raise KeyError like the reference's
    load_imgs / load_vids / load_cats."""
    all_units = np.unique(gt.img_id if unit == "image" else gt.vid_id)
    unit_ids = np.asarray(unit_ids, dtype=np.int64).reshape(-1)
    pos = np.searchsorted(all_units, unit_ids)
    bad = (pos >= len(all_units)) | (all_units[np.minimum(pos, len(all_units) - 1)] != unit_ids) \
        if len(all_units) else np.ones(len(unit_ids), bool)
    if bad.any():
        raise KeyError(int(unit_ids[np.flatnonzero(bad)[0]]))
    all_cats = np.unique(gt.cat_id)
    cat_ids = np.asarray(cat_ids, dtype=np.int64).reshape(-1)
    if len(cat_ids) == 0:
        raise NotImplementedError("an empty params.cat_ids is not evaluated")
    cpos = np.searchsorted(all_cats, cat_ids)
    cbad = (cpos >= len(all_cats)) | (all_cats[np.minimum(cpos, len(all_cats) - 1)] != cat_ids)
    if cbad.any():
        raise KeyError(int(cat_ids[np.flatnonzero(cbad)[0]]))
    whole_cats = len(cat_ids) == len(all_cats) and np.array_equal(cat_ids, all_cats)
    if not whole_cats and not use_cats:
        raise NotImplementedError(
            "params.cat_ids restricts the categories while use_cats = 0 pools "
            "them: not evaluated on the HIP path")
    if len(unit_ids) != len(all_units):
        if unit == "image":
            keep = np.isin(gt.img_id, unit_ids)
            gt = gt.select_images(keep)
            dt = dt.take(np.flatnonzero(np.isin(dt.image_id, unit_ids)))
        else:
            gt = gt.select_videos(np.isin(gt.vid_id, unit_ids))
            # predictions on the images of those videos (T/tao.py:224-235)
            dt = dt.take(np.flatnonzero(np.isin(dt.image_id, gt.img_id)))
    return gt, dt, (None if whole_cats else cpos)


class CellView:
    """What the reference stores per (unit, category, range) in eval_imgs /
    eval_vids, rebuilt on demand from the device results.  ``cat_pos``: index
    of the caller's i-th category (params.cat_ids) in the tables' category
    axis, when params.cat_ids is not the whole sorted table."""

    cat_pos = None

    def __init__(self, run, unit_ids, sentinel, unit_key, rng_key, rng_values):
        self.run = run
        self.flat = run.flat
        self.unit_ids = unit_ids
        self.sentinel = sentinel
        self.unit_key, self.rng_key, self.rng_values = unit_key, rng_key, rng_values
        self.K = len(self.flat.cat_ids)
        self._index = None

    def cell_of(self, unit_idx, cat_idx, table_index=False):
        if self.cat_pos is not None and not table_index:
            cat_idx = self.cat_pos[cat_idx]
        if self._index is None:     # built on first inspection only
            f = self.flat
            self._index = {int(u) * self.K + int(c): k for k, (u, c) in
                           enumerate(zip(f.cell_unit, f.cell_cat))}
        return self._index.get(int(unit_idx) * self.K + int(cat_idx))

    def iou(self, k):
        f, d = self.flat, self.run.detail()
        off = np.zeros(f.n_cells + 1, dtype=np.int64)
        np.cumsum(np.diff(f.cell_dt_off).astype(np.int64)
                  * np.diff(f.cell_gt_off), out=off[1:])
        D = f.cell_dt_off[k + 1] - f.cell_dt_off[k]
        G = f.cell_gt_off[k + 1] - f.cell_gt_off[k]
        if self.flat.kind == "lvis" and (D == 0 or G == 0):
            return []           # mask_utils.iou returns [] (_mask.pyx:203-204)
        return d["iou"][off[k]:off[k + 1]].reshape(D, G).copy()

    def entry(self, k, r):
        f, d = self.flat, self.run.detail()
        d0, d1 = f.cell_dt_off[k], f.cell_dt_off[k + 1]
        g0, g1 = f.cell_gt_off[k], f.cell_gt_off[k + 1]
        D, G = d1 - d0, g1 - g0
        gid = f.gt_id[g0:g1]
        ig = ((d["gt_rng"][g0:g1] >> np.uint32(r)) & np.uint32(1)).astype(np.int64)
        perm = np.argsort(ig, kind="mergesort")
        slots = self.run.thr_slots()
        dt_m = np.full((len(slots), D), float(self.sentinel))
        gt_m = np.full((len(slots), G), float(self.sentinel))
        dt_ig = np.zeros((len(slots), D), dtype=bool)
        for t, slot in enumerate(slots):
            combo = r * N_THR + slot
            m = d["match_gt"][d0:d1, combo]
            hit = m >= 0
            if G:
                dt_m[t, hit] = gid[m[hit]]
                for j in np.flatnonzero(hit):
                    gt_m[t, m[j]] = f.dt_id[d0 + j]
            dt_ig[t] = _bit(d["ignored"][d0:d1], combo)
        return {
            self.unit_key: int(self.unit_ids[f.cell_unit[k]]),
            "category_id": int(f.cat_ids[f.cell_cat[k]]),
            self.rng_key: self.rng_values[r],
            "dt_ids": f.dt_id[d0:d1].tolist(),
            "gt_ids": gid[perm].tolist(),
            "dt_matches": dt_m,
            "gt_matches": gt_m[:, perm],
            "dt_scores": f.dt_score[d0:d1].tolist(),
            "gt_ignore": ig[perm],
            "dt_ignore": dt_ig,
        }


class LazyIous(Mapping):
    """``self.ious``: {(unit_id, cat_id): (D, G) array or []} over ALL unit x
    category pairs, like the reference, but computed on access."""

    def __init__(self, view, unit_list, cat_list):
        self.view, self.units, self.cats = view, unit_list, cat_list
        self._pos = None

    def _positions(self):
        # (600 k images at full scale: built when somebody looks something up)
        if self._pos is None:
            self._pos = ({int(u): i for i, u in enumerate(self.view.unit_ids)},
                         {int(c): i for i, c in enumerate(self.view.flat.cat_ids)})
        return self._pos

    @property
    def upos(self):
        return self._positions()[0]

    @property
    def cpos(self):
        return self._positions()[1]

    def __getitem__(self, key):
        u, c = key
        if u not in self.upos or c not in self.cpos:
            raise KeyError(key)
        k = self.view.cell_of(self.upos[u], self.cpos[c], table_index=True)
        return [] if k is None else self.view.iou(k)

    def __iter__(self):
        return ((int(u), int(c)) for u in self.units for c in self.cats)

    def __len__(self):
        return len(self.units) * len(self.cats)


class LazyPointers(Mapping):
    """eval['dt_pointers'][cat_idx][range...] = {dt_ids, tps, fps}."""

    def __init__(self, run, n_rng, shape, cat_pos=None):
        self.run, self.n_rng, self.shape = run, n_rng, shape
        self.cat_pos = cat_pos
        self._rows = None

    def _data(self):
        if self._rows is None:
            self._rows = self.run.pointer_tables()
        return self._rows

    def leaf(self, k, r):
        d = self._data()
        matched, ignored = d["matched"], d["ignored"]
        if d["num_gt"][k, r] == 0:
            return {}
        lo, hi = int(d["cat_off"][k]), int(d["cat_off"][k + 1])
        slots = self.run.thr_slots()
        m = np.stack([_bit(matched[lo:hi], r * N_THR + t) for t in slots])
        i = np.stack([_bit(ignored[lo:hi], r * N_THR + t) for t in slots])
        return {"dt_ids": d["ids"][lo:hi], "tps": m & ~i, "fps": ~m & ~i}

    def __getitem__(self, k):
        if not 0 <= k < len(self):
            raise KeyError(k)
        if self.cat_pos is not None:
            k = int(self.cat_pos[k])
        if len(self.shape) == 1:
            return {r: self.leaf(k, r) for r in range(self.shape[0])}
        A, T = self.shape
        return {a: {t: self.leaf(k, a * T + t) for t in range(T)}
                for a in range(A)}

    def __iter__(self):
        return iter(range(len(self)))

    def __len__(self):
        return self.run.dp.n_cat if self.cat_pos is None else len(self.cat_pos)


def operating_points(scores, iou_thrs, rec_thrs, cat_ids, iou_thr, recall):
    """{category id: score} at one IoU threshold and one recall threshold from
    scores[T, R, K] (eval["scores"] at one range): the confidence at which the
    category reaches that recall.  The thresholds are looked up like
    _summarize's (exact floats, ``thr == params.iou_thrs``); categories without
    evaluated ground truth (-1) are left out."""
    t = np.where(iou_thr == np.asarray(iou_thrs))[0]
    j = np.where(recall == np.asarray(rec_thrs))[0]
    if len(t) == 0 or len(j) == 0:
        raise ValueError("iou_thr / recall is not one of params.iou_thrs / params.rec_thrs")
    col = np.asarray(scores)[t[0], j[0]]
    return {int(c): float(v) for c, v in zip(cat_ids, col.tolist()) if v != -1}


# The on-request analyses of LVISEval and TaoEval: one body each; the methods
# of the two classes hold the documentation and call these.  What a class `ev`
# supplies: _rng_lbl() = the label of every range; _rng_text(label) = how a
# line names it; _dt_ids() = the column that identifies a row of "dt_type";
# _level = "" / " track", the word of the tables' titles; _cats() = the
# annotation file's categories by id.

def error_key(iou_thrs, iou_thr, bg_thr):
    """(index of `iou_thr` in params.iou_thrs, bg_thr): what the kernels are
    asked for and the key the analyses are cached under.  `iou_thr` is looked
    up like _summarize's; 0 <= bg_thr < tf = min(iou_thr, 1 - 1e-10)."""
    at = np.where(iou_thr == np.asarray(iou_thrs))[0]
    if len(at) == 0:
        raise ValueError("iou_thr: {} is not one of params.iou_thrs".format(iou_thr))
    tf = min(float(np.asarray(iou_thrs)[at[0]]), 1 - 1e-10)
    if not 0 <= bg_thr < tf:
        raise ValueError("bg_thr: {} is not in [0, {})".format(bg_thr, tf))
    return int(at[0]), float(bg_thr)


def _params_cats(ev, table, axis):
    """`table` with its category axis in the order of params.cat_ids."""
    if ev._cat_pos is None:
        return table
    return np.ascontiguousarray(table[(slice(None),) * axis + (ev._cat_pos,)])


def score_at_recall(ev):
    if not ev.eval:
        raise RuntimeError("Please run accumulate() first.")
    if "scores" not in ev.eval:
        scores = _params_cats(ev, ev._run.score_table(), 2)
        # (the track level's two range axes; the image level's shape as it is)
        ev.eval["scores"] = scores.reshape(ev.eval["precision"].shape)
    return ev.eval["scores"]


def error_types(ev, iou_thr, bg_thr, per_detection):
    if ev._run is None:
        raise RuntimeError("Please run evaluate() first.")
    key = error_key(ev.params.iou_thrs, iou_thr, bg_thr)
    hit = ev._error_types.get(key)
    if hit is None or (per_detection and "dt_type" not in hit):
        dt_counts, gt_counts, dt_type = ev._run.error_table(key[0], key[1], per_detection)
        from .._lib import ERROR_TYPES
        hit = {"types": list(ERROR_TYPES), "dt_counts": _params_cats(ev, dt_counts, 1),
               "gt_counts": _params_cats(ev, gt_counts, 1), "rng_lbl": ev._rng_lbl()}
        if per_detection:
            hit["dt_type"] = (ev._dt_ids(), dt_type)
        ev._error_types[key] = hit
    return hit if per_detection else {k: v for k, v in hit.items() if k != "dt_type"}


def error_impact(ev, iou_thr, bg_thr):
    if ev._run is None:
        raise RuntimeError("Please run evaluate() first.")
    key = error_key(ev.params.iou_thrs, iou_thr, bg_thr)
    hit = ev._error_impact.get(key)
    if hit is None:
        precision = _params_cats(ev, ev._run.impact_table(key[0], key[1])[0], 2)
        from .._lib import ERROR_FIXES
        ap = np.array([[masked_mean(precision[v, :, :, a])
                        for a in range(precision.shape[3])]
                       for v in range(precision.shape[0])], dtype=np.float64)
        hit = {"fixes": list(ERROR_FIXES), "precision": precision, "ap": ap,
               "dap": ap[1:] - ap[0], "rng_lbl": ev._rng_lbl()}
        ev._error_impact[key] = hit
    return dict(hit)


def _title(ev, what, iou_thr, bg_thr, more=""):
    """The title line of an analysis' text table."""
    return "{} {} @[ IoU={:0.2f} | bg={:0.2f}{} ]".format(ev._level, what, iou_thr, bg_thr, more)


def _range_name(ev, e, a):
    """How a line names range `a`; a range past the labels goes by its index."""
    return ev._rng_text(e["rng_lbl"][a]) if a < len(e["rng_lbl"]) else str(a)


def _range_lines(ev, e, what, iou_thr, bg_thr, cols, rows, cell):
    """A title, the column names and a line per range (row of `rows`), every
    value through the format `cell`; a range past the labels goes by its index."""
    lbl = [_range_name(ev, e, a) for a in range(len(rows))]
    w = max([len(x) for x in lbl] + [10])
    width = len(cell.format(0))         # the column names as wide as the cells
    lines = [_title(ev, what, iou_thr, bg_thr),
             " " + " " * w + "".join(c.rjust(width) for c in cols)]
    for name, r in zip(lbl, rows):
        lines.append(" " + name.ljust(w) + "".join(cell.format(v) for v in r.tolist()))
    return lines


def error_lines(ev, iou_thr, bg_thr):
    e = ev.error_types(iou_thr, bg_thr)
    rows = np.concatenate([e["dt_counts"].sum(1), e["gt_counts"].sum(1)], axis=1)
    return _range_lines(ev, e, "error types", iou_thr, bg_thr,
                        e["types"] + ["GT", "missed", "missed_loc"], rows, "{:>11d}")


def impact_lines(ev, iou_thr, bg_thr):
    e = ev.error_impact(iou_thr, bg_thr)
    rows = np.concatenate([e["ap"][:1], e["dap"]]).T
    return _range_lines(ev, e, "error impact", iou_thr, bg_thr,
                        ["AP"] + ["d" + name for name in e["fixes"][1:]], rows, "{:>9.4f}")


def confusion(ev, iou_thr, bg_thr):
    if ev._run is None:
        raise RuntimeError("Please run evaluate() first.")
    key = error_key(ev.params.iou_thrs, iou_thr, bg_thr)
    hit = ev._confusion.get(key)
    if hit is None:
        rng, dt_cat, gt_cat, counts, K = ev._run.confusion_table(key[0], key[1])
        ids = np.asarray(ev.params.cat_ids, dtype=np.int64).reshape(-1)
        if ev._cat_pos is not None:
            # table category -> its place in params.cat_ids; the others are not asked for
            place = np.full(K, -1, dtype=np.int64)
            place[ev._cat_pos] = np.arange(len(ev._cat_pos))
            dt_cat, gt_cat = place[dt_cat], place[gt_cat]
            keep = np.flatnonzero((dt_cat >= 0) & (gt_cat >= 0))
            keep = keep[np.lexsort((gt_cat[keep], dt_cat[keep], rng[keep]))]
            rng, dt_cat, gt_cat, counts = rng[keep], dt_cat[keep], gt_cat[keep], counts[keep]
        from .._lib import CONFUSION_COLUMNS
        hit = {"columns": list(CONFUSION_COLUMNS), "rng_lbl": ev._rng_lbl(), "rng": rng,
               "dt_cat": ids[dt_cat], "gt_cat": ids[gt_cat], "counts": counts}
        ev._confusion[key] = hit
    return dict(hit)


def confusion_matrix(ev, iou_thr, bg_thr, rng, column):
    e = ev.confusion(iou_thr, bg_thr)
    if column not in e["columns"]:
        raise ValueError("column: {!r} is not one of {}".format(column, e["columns"]))
    ids = np.asarray(ev.params.cat_ids, dtype=np.int64).reshape(-1)
    place = {int(c): i for i, c in enumerate(ids.tolist())}
    sel = np.flatnonzero(e["rng"] == rng)
    out = np.zeros((len(ids), len(ids)), dtype=np.int64)
    at = [place[c] for c in e["dt_cat"][sel].tolist()]
    to = [place[c] for c in e["gt_cat"][sel].tolist()]
    out[at, to] = e["counts"][sel, e["columns"].index(column)]
    return out


def confusion_lines(ev, iou_thr, bg_thr, rng, top):
    e = ev.confusion(iou_thr, bg_thr)
    sel = np.flatnonzero(e["rng"] == rng)
    cols = e["columns"]
    n = e["counts"][sel]
    # most adopted first, then most CLS rows; the entries come by (dt_cat, gt_cat)
    # places, the ids break what ties remain: a total order
    by = np.lexsort((e["gt_cat"][sel], e["dt_cat"][sel], -n[:, cols.index("cls")],
                     -n[:, cols.index("adopted")]))
    sel = sel[by[:max(int(top), 0)]]
    cats = ev._cats()

    def name(c):
        got = cats.get(c, {}).get("name")
        return str(c) if got is None else str(got)
    dt = [(int(c), name(int(c))) for c in e["dt_cat"][sel].tolist()]
    gt = [(int(c), name(int(c))) for c in e["gt_cat"][sel].tolist()]
    wd = max([len(x) for _, x in dt] + [len("predicted")])
    wg = max([len(x) for _, x in gt] + [len("ground truth")])
    lines = [_title(ev, "confusion", iou_thr, bg_thr, " | rng={}".format(_range_name(ev, e, rng))),
             " " + "id".rjust(8) + " " + "predicted".ljust(wd) + " " + "id".rjust(8) + " "
             + "ground truth".ljust(wg) + "".join(c.rjust(9) for c in cols)]
    for (d, dn), (g, gn), r in zip(dt, gt, e["counts"][sel].tolist()):
        lines.append(" {:>8d} {} {:>8d} {}".format(d, dn.ljust(wd), g, gn.ljust(wg))
                     + "".join("{:>9d}".format(v) for v in r))
    return lines


def now():
    return datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S")


class EvalConstants:
    """``params.iou_thrs`` / ``rec_thrs`` and the range tables as the kernels
    take them.  The reference reads all of them when it runs (L/eval.py:140-145,
    205,234,319-329,407; T/eval.py:271-276,385,473-477,562), so a caller may
    edit them before ``run()`` -- values, order AND number.

    The kernels take N_THR IoU thresholds and N_REC recall thresholds per pass,
    ascending, as by-value arguments, and the range VALUES likewise
    (taoamd_set_thresholds / taoamd_set_ranges); the NUMBER of ranges per pass
    is theirs (5 visibility ranges + the out-of-frame one -- the reference's
    LAST range, whatever its bounds, L/eval.py:143 --; 4 areas + the occlusion
    one -- the LAST area range, T/eval.py:272 -- x 4 durations).  Every
    threshold and every range is evaluated independently of the others, so
    the caller's arrays -- any number, any order -- are cut into blocks, a
    short block padded with copies of its last value, a pass runs per block
    and every block's slice of the tables goes where the caller's order has
    it (``rng_blocks``: the tables of a pass and, per kernel range slot, the
    caller's range index)."""

    def __init__(self, params, fresh, kind):
        iou = np.asarray(params.iou_thrs, dtype=np.float64).reshape(-1)
        rec = np.asarray(params.rec_thrs, dtype=np.float64).reshape(-1)
        self.T, self.R = len(iou), len(rec)
        if self.T == 0 or self.R == 0:
            raise NotImplementedError("empty params.iou_thrs / params.rec_thrs")
        if np.isnan(iou).any() or np.isnan(rec).any():
            raise ValueError("params.iou_thrs / params.rec_thrs hold a NaN")
        same = np.array_equal(iou, fresh.iou_thrs) and np.array_equal(rec, fresh.rec_thrs)

        def table(name):
            try:
                got = np.asarray(getattr(params, name), dtype=np.float64)
            except (TypeError, ValueError):
                got = np.zeros(0)
            if got.ndim != 2 or got.shape[1] != 2 or len(got) == 0:
                raise NotImplementedError(
                    "params.%s: a non-empty list of [lo, hi] pairs is evaluated" % name)
            return got, np.asarray(getattr(fresh, name), dtype=np.float64)

        def cut(idx, cap, values, filler):
            """Blocks of <= cap of the ranges `idx`: (indices, (cap, 2) values
            padded with the block's last range)."""
            out = []
            for i in range(0, max(len(idx), 1), cap):
                sel = idx[i:i + cap]
                v = values[sel] if len(sel) else np.zeros((0, 2))
                pad = v[-1:] if len(sel) else filler[None]
                out.append((list(sel), np.concatenate([v] + [pad] * (cap - len(sel)))))
            return out

        self.rng_blocks = []
        if kind == "lvis":
            got, want = table("visibility_rng")
            self.n_rng = len(got)
            # (the last range is the out-of-frame one, its bounds are never
            # read -- L/eval.py:143,209-217)
            same = same and got.shape == want.shape and np.array_equal(got[:-1], want[:-1])
            for b, (sel, vals) in enumerate(cut(np.arange(len(got) - 1), 5, got,
                                                 np.array([0.0, 1.0]))):
                slots = [(k, int(i)) for k, i in enumerate(sel)]
                if b == 0:
                    slots.append((5, len(got) - 1))
                self.rng_blocks.append(({"visibility_rng": vals}, slots))
            identity = len(got) == 6
        else:
            area, want_a = table("area_rng")
            time_, want_t = table("time_rng")
            A, Tm = len(area), len(time_)
            self.n_rng = A * Tm
            same = same and area.shape == want_a.shape and time_.shape == want_t.shape \
                and np.array_equal(area, want_a) and np.array_equal(time_, want_t)
            a_blocks = cut(np.arange(A - 1), 4, area, area[-1])
            t_blocks = cut(np.arange(Tm), 4, time_, time_[-1])
            for ab, (asel, avals) in enumerate(a_blocks):
                # slot 4 of the kernels' area table: the occlusion range
                atab = np.concatenate([avals, area[-1:]])
                aslots = [(k, int(i)) for k, i in enumerate(asel)]
                if ab == 0:
                    aslots.append((4, A - 1))
                for tsel, tvals in t_blocks:
                    slots = [(ka * 4 + kt, ia * Tm + int(it)) for ka, ia in aslots
                             for kt, it in enumerate(tsel)]
                    self.rng_blocks.append(({"area_rng": atab, "time_rng": tvals}, slots))
            identity = A == 5 and Tm == 4
        self.default = bool(same)
        self.thr_blocks = self._blocks(iou, N_THR)
        self.rec_blocks = self._blocks(rec, N_REC)
        # one pass whose tables are the caller's, slot for slot: the per-cell
        # views (ious, eval_imgs / eval_vids, dt_pointers) read such a pass
        self.single = len(self.thr_blocks) == 1 and len(self.rec_blocks) == 1 \
            and len(self.rng_blocks) == 1 and identity
        self.rec_sorted = bool(np.all(np.diff(rec) >= 0))
        self.ranges = self.rng_blocks[0][0]

    @staticmethod
    def _blocks(values, cap):
        order = np.argsort(values, kind="stable")
        out = []
        for i in range(0, len(values), cap):
            idx = order[i:i + cap]
            v = values[idx]
            out.append((idx, np.concatenate([v, np.full(cap - len(v), v[-1])])))
        return out


def applied(constants, thr_block=0, rec_block=0, rng_block=0):
    """Context manager: the calling thread's kernels launched inside take
    ``constants`` (None: nothing to do); the reference's defaults come back on
    the way out."""
    import contextlib
    from .. import _lib

    @contextlib.contextmanager
    def cm():
        if constants is None or constants.default:
            yield
            return
        _lib.set_constants(iou_thrs=constants.thr_blocks[thr_block][1],
                           rec_thrs=constants.rec_blocks[rec_block][1],
                           **constants.rng_blocks[rng_block][0])
        try:
            yield
        finally:
            _lib.set_constants()
    return cm()
