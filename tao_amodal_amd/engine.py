"""Device pipeline: flattened cell tables -> precision / recall on the GPU.

PyTorch is used only as the allocator/stream provider (device tensors,
``data_ptr()``, ``torch.cuda.current_stream()``); every arithmetic step is a
hand-written HIP kernel behind the C ABI of ``include/tao_amodal_hip.h``.

One evaluator pass ("step" of bench.py) =

    ranges  ->  sort (category, -score)  ->  [track 3D IoU]  ->
    IoU + greedy match (writes rows in sorted order)  ->  accumulate

which covers reference LVISEval.evaluate()+accumulate() (lvis_amodal/eval.py:
115-145,305-426) or TaoEval.evaluate()+accumulate() (tao_amodal/eval.py:
246-276,459-584) for the non-empty cells.
"""
import os

import numpy as np
import torch

from . import _lib

N_THR, N_REC = _lib.N_THR, _lib.N_REC


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _to_device(v, device):
    """Upload a table of a flattened problem.  flatten.LazyRows (rows of a raw
    input table) are gathered on the device from ONE upload of the raw table
    (flatten_dev.device_copy), shared by every problem built from the same input."""
    from .flatten import LazyRows
    if not isinstance(v, LazyRows):
        return torch.from_numpy(np.ascontiguousarray(v)).to(device)
    from .flatten_dev import device_copy
    src = device_copy(v.source, device)
    if len(v.index) == 0:
        return torch.zeros((0,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    return src.index_select(0, torch.from_numpy(v.index).to(src.device))


def match_plan(cell_dt_off, cell_gt_off, cap_d=64, cap_g=64, cap_cell_g=8):
    """Pack runs of consecutive small cells (<= cap_d detections and <= cap_g
    GTs in total, <= cap_cell_g GTs per cell) into groups for
    match_group_kernel; every other cell that has detections is a 'single'
    (taoamd_match_plan_host)."""
    lib = _lib.load()
    d_off = np.ascontiguousarray(cell_dt_off, dtype=np.int32)
    g_off = np.ascontiguousarray(cell_gt_off, dtype=np.int32)
    sizes = np.zeros(2, dtype=np.int64)
    args = (len(d_off) - 1, d_off.ctypes.data, g_off.ctypes.data, cap_d, cap_g,
            cap_cell_g, sizes.ctypes.data)
    _lib.check(lib.taoamd_match_plan_host(*args, None, None),
               "taoamd_match_plan_host")
    ng, ns = int(sizes[0]), int(sizes[1])
    groups = np.zeros((max(ng, 1), 2), dtype=np.int32)
    singles = np.zeros(max(ns, 1), dtype=np.int32)
    if ng or ns:
        _lib.check(lib.taoamd_match_plan_host(
            *args, groups.ctypes.data, singles.ctypes.data),
            "taoamd_match_plan_host")
    return groups[:ng], singles[:ns]


def sort_plan(cat_off):
    """Chunks / buckets / scatter tiles of taoamd_sort_sampled from the host
    copy of the category offsets (taoamd_sort_plan_host).  Returns the four
    int32 tables and whether some category needs the merge passes."""
    lib = _lib.load()
    off = np.ascontiguousarray(cat_off, dtype=np.int32)
    sizes = np.zeros(5, dtype=np.int64)
    _lib.check(lib.taoamd_sort_plan_host(len(off) - 1, off.ctypes.data,
                                         sizes.ctypes.data, None, None, None, None),
               "taoamd_sort_plan_host")
    nc, ns, nt, nb = (int(x) for x in sizes[:4])
    chunks = np.zeros((max(nc, 1), 8), dtype=np.int32)
    split = np.zeros(max(ns, 1), dtype=np.int32)
    stile = np.zeros(max(nt, 1), dtype=np.int32)
    bucket = np.zeros(max(nb, 1), dtype=np.int32)
    if nc:
        _lib.check(lib.taoamd_sort_plan_host(
            len(off) - 1, off.ctypes.data, sizes.ctypes.data, chunks.ctypes.data,
            split.ctypes.data, stile.ctypes.data, bucket.ctypes.data),
            "taoamd_sort_plan_host")
    return (chunks, split, stile, bucket), (nc, ns, nt, nb), bool(sizes[4])


def track_meta(flat):
    """{first, last, base - first, is detection} of every track (detection
    tracks first, then GT) for the padded frame table: track t owns the slots
    base .. base + last - first; slot 0 is the table's far box.  Returns the
    int32 table, the slot range of either side and the table size."""
    metas, sides, n_slots = [], {}, 1
    for side in ("dt", "gt"):
        dev = getattr(flat, "dev", {})
        if side + "_frame_off" in dev and side + "_frame_pos" in dev \
                and not dict.__contains__(flat, side + "_frame_pos"):
            # device-built tables: the tracks' first / last positions are
            # gathered where the frame lists are (21 M positions at the
            # validation scale: 0.04 s to bring them to the host for this)
            off_t, pos_t = dev[side + "_frame_off"].long(), dev[side + "_frame_pos"]
            has_t = off_t[1:] > off_t[:-1]
            top = max(int(pos_t.numel()) - 1, 0)
            if pos_t.numel():
                first_t = torch.where(has_t, pos_t[off_t[:-1].clamp(max=top)].long(),
                                      torch.ones_like(off_t[1:]))
                last_t = torch.where(has_t, pos_t[(off_t[1:] - 1).clamp(min=0, max=top)].long(),
                                     torch.zeros_like(off_t[1:]))
            else:
                first_t, last_t = torch.ones_like(off_t[1:]), torch.zeros_like(off_t[1:])
            both = torch.stack([first_t, last_t]).cpu().numpy()
            first, last = both[0], both[1]
            has = last >= first
        else:
            off = np.asarray(flat[side + "_frame_off"], dtype=np.int64)
            pos = np.asarray(flat[side + "_frame_pos"], dtype=np.int64)
            has = off[1:] > off[:-1]
            first = np.ones(len(off) - 1, dtype=np.int64)
            last = np.zeros(len(off) - 1, dtype=np.int64)
            first[has] = pos[off[:-1][has]]
            last[has] = pos[off[1:][has] - 1]
        span = np.where(has, last - first + 1, 0)
        base = n_slots + np.cumsum(span) - span
        metas.append(np.stack([first, last, base - first,
                               np.full_like(first, side == "dt")], 1))
        total = int(span.sum())
        # the first set also fills slot 0
        sides[side] = (n_slots - (side == "dt"), total + (side == "dt"))
        n_slots += total
    return np.concatenate(metas), sides, n_slots


def _track_iou_plan(flat, meta, spans):
    """The two-call protocol of the plan functions: sizes, then the tables."""
    lib = _lib.load()
    name = "taoamd_track_iou_plan_spans_host" if spans else "taoamd_track_iou_plan_host"
    d_off = np.ascontiguousarray(flat.cell_dt_off, dtype=np.int32)
    g_off = np.ascontiguousarray(flat.cell_gt_off, dtype=np.int32)
    i_off = np.ascontiguousarray(flat.cell_iou_off, dtype=np.int64)
    meta = np.ascontiguousarray(meta, dtype=np.int32)
    sizes = np.zeros(4 if spans else 3, dtype=np.int64)
    args = (len(d_off) - 1, d_off.ctypes.data, g_off.ctypes.data,
            i_off.ctypes.data, meta.ctypes.data, sizes.ctypes.data)
    _lib.check(getattr(lib, name)(*args, *([None] * (5 if spans else 4))), name)
    tabs = [np.zeros((int(sizes[0]), 4), dtype=np.int32),
            np.zeros(int(sizes[1]), dtype=np.int32),
            np.zeros(int(sizes[2]), dtype=np.int32),
            np.zeros(int(sizes[2]), dtype=np.int64)]
    if spans:
        tabs.append(np.zeros(int(sizes[3]), dtype=np.int64))
    if sizes[0] or (spans and sizes[3]):
        _lib.check(getattr(lib, name)(*args, *(t.ctypes.data for t in tabs)), name)
    return tuple(tabs)


def track_iou_plan(flat, meta):
    """Launch plan of taoamd_track_iou_planned with every pair in a task (one
    wavefront per task: up to 32 tracks, up to 64 track pairs).  Returns
    tasks[n, 4], task_rows, task_pairs (int32) and task_out (int64)."""
    return _track_iou_plan(flat, meta, False)


def track_iou_plan_spans(flat, meta):
    """The span-aware launch plan (taoamd_track_iou_plan_spans_host), the one
    the engine uses: pairs of two tracks whose spans first .. last share no
    position are +0.0 in every mode and go to a zero list instead of a task.
    Returns tasks[n, 4], task_rows, task_pairs (int32), task_out and zero_out
    (int64)."""
    return _track_iou_plan(flat, meta, True)


class DeviceProblem:
    """A flattened problem (flatten.Flat) resident in HBM."""

    IOU_MODES = {"3d_iou": 0, "avg_iou": 1, "imagenetvid": 2}

    def __init__(self, flat, device="cuda", iou_3d_type="3d_iou", guard="device"):
        """`guard`: where the frame-order guard recomputes the listed pairs --
        "device" (taoamd_track_iou_setorder, no host round trip; falls back to
        the host when an image id is outside [0, 2^61 - 1)) or "host" (Python's
        own sets, one synchronisation per pass: the cross-check of the tests)."""
        self.kind = flat.kind
        self.iou_mode = self.IOU_MODES[iou_3d_type]
        self.device = torch.device(device)
        self.n_rng = _lib.LVIS_RNG if self.kind == "lvis" else _lib.TAO_RNG
        self.n_words = (self.n_rng * N_THR + 63) // 64
        self.n_cells = int(flat.n_cells)
        self.n_cat = len(flat.cat_ids)
        self.n_dt = int(flat.cell_dt_off[-1])
        self.n_gt = int(flat.cell_gt_off[-1])
        self.n_pairs = int(flat.n_pairs)
        # image / video of every cell (host): the error breakdown groups rows by it
        self.cell_unit_host = flat.get("cell_unit")
        # its per-unit row lists, built by the first breakdown (_error_tabs), and
        # the image level's column beside them
        self.err_tabs = self.err_dt_gt0 = None
        # tables a device-side build (flatten_dev.DeviceFlat) already holds in HBM
        on_dev = getattr(flat, "dev", {})
        d_cnt = np.diff(flat.cell_dt_off).astype(np.int64)
        g_cnt = np.diff(flat.cell_gt_off).astype(np.int64)
        self.max_g = int(g_cnt.max()) if self.n_cells else 0
        if self.max_g > _lib.MAX_GT_PER_CELL:
            raise _lib.TaoAmdError(
                "a cell holds %d ground truths; the kernels support up to %d"
                % (self.max_g, _lib.MAX_GT_PER_CELL))
        iou_off = np.zeros(self.n_cells + 1, dtype=np.int64)
        np.cumsum(d_cnt * g_cnt, out=iou_off[1:])
        self.n_iou = int(iou_off[-1])
        # category-major cells (flatten.py): every category is one run of
        # cells, of detections and of ground truths
        cell_cat = np.asarray(flat.cell_cat)
        self.grouped = bool(np.all(np.diff(cell_cat) >= 0))
        if self.grouped:
            first = np.searchsorted(cell_cat, np.arange(self.n_cat + 1), "left")
            cat_off = np.asarray(flat.cell_dt_off)[first].astype(np.int32)
            gt_cat_off = np.asarray(flat.cell_gt_off)[first].astype(np.int32)
        else:
            cat_off = np.zeros(self.n_cat + 1, dtype=np.int32)
            np.cumsum(np.bincount(flat.dt_cat, minlength=self.n_cat),
                      out=cat_off[1:])
            gt_cat_off = np.zeros(self.n_cat + 1, dtype=np.int32)
            np.cumsum(np.bincount(flat.gt_cat, minlength=self.n_cat),
                      out=gt_cat_off[1:])
        groups, singles = match_plan(flat.cell_dt_off, flat.cell_gt_off)
        self.n_groups, self.n_singles = len(groups), len(singles)
        names = ["cell_dt_off", "cell_gt_off", "dt_score", "dt_flags",
                 "dt_cat", "gt_flags", "gt_cat", "dt_cell"]
        if self.kind == "lvis":
            names += ["dt_box", "gt_box", "gt_vis"]
        else:
            names += ["dt_area", "dt_len", "gt_area", "gt_len", "gt_nhp",
                      "dt_frame_off", "dt_frame_pos", "dt_frame_box",
                      "gt_frame_off", "gt_frame_pos", "gt_frame_box"]
        self.t = {}
        for n in names:
            self.t[n] = on_dev[n].to(self.device) if n in on_dev else \
                _to_device(flat[n], self.device)
        # iou_type="segm": run-length masks (masks.MaskArrays), row i = detection
        # / ground truth i of the tables (image level) or frame i of the
        # *_frame_* lists (track level); the IoU then comes from taoamd_rle_iou
        # / taoamd_track_mask_iou instead of the boxes
        masks = flat.get("masks")
        self.mask_iou = masks is not None
        self.rle_total, self.rle_rows = {}, {}
        if self.mask_iou:
            self.rle_total = {k: int(masks[k].off[-1]) for k in ("dt", "gt")}
            rows = (("dt", self.n_dt), ("gt", self.n_gt)) if self.kind == "lvis" else \
                (("dt", int(self.t["dt_frame_pos"].numel())),
                 ("gt", int(self.t["gt_frame_pos"].numel())))
            self.rle_rows = dict(rows)
            for side, n_rows in rows:
                m = masks[side]
                if len(m) != n_rows:
                    raise _lib.TaoAmdError(
                        "%d %s masks for %d rows" % (len(m), side, n_rows))
                self.t[side + "_rle_off"] = torch.from_numpy(m.off).to(self.device)
                self.t[side + "_rle_runs"] = torch.from_numpy(
                    np.ascontiguousarray(m.counts if len(m.counts) else
                                         np.zeros(1, np.uint32)).view(np.int32)
                ).to(self.device)
                self.t[side + "_rle_hw"] = torch.from_numpy(
                    np.ascontiguousarray(m.hw).reshape(-1, 2) if len(m) else
                    np.zeros((1, 2), np.int32)).to(self.device)
                self.t[side + "_rle_bb"] = torch.from_numpy(
                    np.ascontiguousarray(m.bbox).reshape(-1, 4) if len(m) else
                    np.zeros((1, 4))).to(self.device)
        self.max_segment = int(np.diff(cat_off).max()) if self.n_cat else 0
        # hint for the sweep: longest category (0 = unknown -> chunked kernels)
        self.acc_hint = self.max_segment
        tiles = (np.diff(cat_off) + _lib.SEGMENT_TILE - 1) // _lib.SEGMENT_TILE
        tile_off = np.zeros(self.n_cat + 1, dtype=np.int32)
        np.cumsum(tiles, out=tile_off[1:])
        self.n_tiles = int(tile_off[-1])
        # run descriptors {first detection, detections, first GT, GTs}
        runs = np.zeros((max(len(groups), 1), 4), dtype=np.int32)
        if len(groups):
            c0, c1 = groups[:, 0], groups[:, 1]
            runs[:, 0] = flat.cell_dt_off[c0]
            runs[:, 1] = flat.cell_dt_off[c1] - flat.cell_dt_off[c0]
            runs[:, 2] = flat.cell_gt_off[c0]
            runs[:, 3] = flat.cell_gt_off[c1] - flat.cell_gt_off[c0]
        self.t["groups"] = torch.from_numpy(runs).to(self.device)
        # (host copies: the multi-GPU plan cuts the launch plan into phases)
        self.groups_host = runs[:len(groups)]
        self.singles_host = np.asarray(singles, dtype=np.int32)
        self.singles_first_dt = np.asarray(flat.cell_dt_off)[self.singles_host] \
            if len(singles) else np.zeros(0, np.int32)
        self.n_tasks = 0
        self.single_frame = False
        self.exact_terms = False
        self.guard_flat = None         # host tables of the host-side guard
        self.guard_on_device = False
        self.near_ulp = 0
        if self.kind == "tao":
            self._plan_track_iou(flat)
            self._plan_guard(flat, guard)
        # per detection {first GT of its cell, GT count, position in the cell,
        # cell}: resolved here, on the device, from the uploaded cell tables
        cell = self.t["dt_cell"].long()
        g_off, d_off = self.t["cell_gt_off"], self.t["cell_dt_off"]
        self.t["dt_group"] = torch.stack(
            [g_off[cell], g_off[cell + 1] - g_off[cell],
             torch.arange(self.n_dt, dtype=torch.int32, device=self.device)
             - d_off[cell], self.t["dt_cell"]], dim=1).to(torch.int32).contiguous() \
            if self.n_dt else torch.zeros((1, 4), dtype=torch.int32,
                                          device=self.device)
        # image level: the same (relative to the run's first GT) and the flag
        # byte packed into one word per detection, all the group kernel reads
        # when it computes the IoUs itself (taoamd_match: dt_meta)
        self.t["dt_meta"] = None
        if self.kind == "lvis" and not self.mask_iou and self.n_dt and len(groups):
            dg, runs_t = self.t["dt_group"], self.t["groups"]
            d = torch.arange(self.n_dt, dtype=torch.int32, device=self.device)
            rid = (torch.searchsorted(runs_t[:, 0].contiguous(), d, right=True) - 1
                   ).clamp_(min=0)
            self.t["dt_meta"] = (
                self.t["dt_flags"].to(torch.int32)
                | (((dg[:, 0] - runs_t[:, 2][rid]) & 63) << 8)
                | (dg[:, 1].clamp(max=15) << 14) | ((dg[:, 2] & 63) << 18)).contiguous()
        self.t["singles"] = torch.from_numpy(
            singles if len(singles) else np.zeros(1, np.int32)).to(self.device)
        self.t["cell_iou_off"] = torch.from_numpy(iou_off).to(self.device)
        self.t["cat_off"] = torch.from_numpy(cat_off).to(self.device)
        self.t["gt_cat_off"] = torch.from_numpy(gt_cat_off).to(self.device)
        self.t["tile_off"] = torch.from_numpy(tile_off).to(self.device)
        self.cat_off_host = cat_off
        # plan of the sample sort (depends on cat_off alone)
        self.ss_sizes, self.ss_merge = (0, 0, 0, 0), False
        if self.grouped and self.n_dt:
            tabs, self.ss_sizes, self.ss_merge = sort_plan(cat_off)
            for name, tab in zip(("ss_chunks", "ss_split", "ss_stile", "ss_bucket"), tabs):
                self.t[name] = torch.from_numpy(tab).to(self.device)

    def _plan_track_iou(self, flat):
        """Padded frame table + launch plan of taoamd_track_iou_planned."""
        lib = _lib.load()
        self._drop_plan()
        if self.device.type != "cuda":     # host-side plumbing tests: no kernels
            return
        if self.mask_iou:                  # taoamd_track_mask_iou: no plan
            return
        meta, sides, n_slots = track_meta(flat)
        n_frames = sum(int(getattr(flat, "dev", {})[k].numel())
                       if k in getattr(flat, "dev", {}) and not dict.__contains__(flat, k)
                       else len(flat[k]) for k in ("dt_frame_pos", "gt_frame_pos"))
        self.n_slots = n_slots
        # tracks that are mostly holes would blow the table up: such inputs
        # take the two-pointer merge kernel instead (no plan)
        if n_slots > 4 * n_frames + (1 << 20) or n_slots >= 2 ** 31 - 1:
            return
        # every track a single frame (the stress shape: 10 000 one-frame
        # videos): a pair is ONE box IoU or 0 -- no sum, no order of summation,
        # nothing to guard; taoamd_track_iou_single instead of the task kernel,
        # whose LDS pipeline would be all prologue (1.05 ms for 2.9 M tracks)
        self.single_frame = (len(meta) > 0 and n_frames == len(meta)
                             and bool((meta[:, 0] == meta[:, 1]).all())
                             and os.environ.get("TAOAMD_SINGLE_FRAME", "1") != "0")
        if self.single_frame:
            self.exact_terms = True
            return
        tasks, rows, pairs, out, zero = track_iou_plan_spans(flat, meta)
        self.n_tasks = len(tasks)
        if self.n_tasks == 0:
            return
        dev = self.device
        self.t["tasks"] = torch.from_numpy(tasks).to(dev)
        self.t["task_rows"] = torch.from_numpy(rows).to(dev)
        self.t["task_pairs"] = torch.from_numpy(pairs).to(dev)
        self.t["task_out"] = torch.from_numpy(out).to(dev)
        self.t["zero_out"] = torch.from_numpy(zero).to(dev)
        self.t["trk_meta"] = torch.from_numpy(
            np.ascontiguousarray(meta, dtype=np.int32)).to(dev)
        padded = torch.empty((n_slots, 4), dtype=torch.float64, device=dev)
        # (sizes from the device tensors: a device-built table would bring its
        # frame lists to the host to answer len())
        n_dt = int(self.t["dt_frame_off"].numel()) - 1
        inexact = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            for side, row0 in (("dt", 0), ("gt", n_dt)):
                slot0, slots = sides[side]
                n_trk = int(self.t[side + "_frame_off"].numel()) - 1
                _lib.check(lib.taoamd_track_pad(
                    n_trk, int(self.t[side + "_frame_pos"].numel()),
                    _ptr(self.t[side + "_frame_off"]),
                    _ptr(self.t[side + "_frame_pos"]),
                    _ptr(self.t[side + "_frame_box"]),
                    self.t["trk_meta"].data_ptr() + 16 * row0, slot0, slots,
                    _ptr(padded), _ptr(inexact), _stream()),
                    "taoamd_track_pad")
            # the frames in the order the tasks read them (taoamd_track_stream):
            # a row owns a 256-byte piece in every 8-position chunk its span
            # reaches into; a task's pieces lie chunk by chunk, rows in order
            has = meta[:, 1] >= meta[:, 0]
            trk_pieces = np.where(has, (meta[:, 1] >> 3) - (meta[:, 0] >> 3) + 1, 0)
            task_pieces = np.add.reduceat(trk_pieces[rows].astype(np.int64),
                                          tasks[:, 0].astype(np.int64))
            base = 1 + np.cumsum(task_pieces) - task_pieces
            n_pieces = 1 + int(task_pieces.sum())
            # (a task's stretch is addressed by 32-bit byte offsets)
            if n_pieces >= 2 ** 31 - 1 or int(task_pieces.max()) * 256 >= 2 ** 32:
                self._drop_plan()           # (the plan-less kernel takes over)
                return
            self.t["task_base"] = torch.from_numpy(base.astype(np.int32)).to(dev)
            # (+ a margin behind the last piece: a stager lane whose row has no
            # piece in a chunk loads from behind the chunk's stretch)
            self.t["frames"] = torch.empty(((n_pieces + 64) * 8, 4), dtype=torch.float64,
                                           device=dev)
            _lib.check(lib.taoamd_track_stream(
                self.n_tasks, _ptr(self.t["tasks"]), _ptr(self.t["task_rows"]),
                _ptr(self.t["trk_meta"]), _ptr(self.t["task_base"]), _ptr(padded),
                _ptr(self.t["frames"]), _stream()), "taoamd_track_stream")
            del padded
        # integer boxes: frame sums are exact in any order, nothing to guard
        # (products < 2^40, tracks of at most 2^12 frames: every sum < 2^53)
        longest = int((meta[:, 1] - meta[:, 0]).max()) + 1 if len(meta) else 0
        flags = int(inexact.item())
        self.exact_terms = not (flags & 1) and longest <= 4096
        # a corner at or beyond the far box's 1e300, or not finite: the task
        # kernel's sentinel would not be out of band (the plan-less kernel
        # takes over: it has none)
        if flags & 2:
            self._drop_plan()

    PLAN_TABLES = ("tasks", "task_rows", "task_pairs", "task_out", "frames",
                   "task_base", "trk_meta", "zero_out")

    def _drop_plan(self):
        """No launch plan: stage_track_iou takes the plan-less merge kernel."""
        for k in self.PLAN_TABLES:
            self.t[k] = None

    def guard_active(self):
        """Whether a pass runs the frame-order guard: the count-based
        imagenetvid IoU is exact in any order, and so is the 3D IoU of integer
        boxes (exact_terms) -- but NOT the average IoU of integer boxes, whose
        per-frame ratios are rounded divisions.  One-frame tracks have a
        single term in every mode."""
        return (self.kind == "tao" and self.n_iou > 0 and self.iou_mode != 2
                and not self.mask_iou
                and not (self.exact_terms and self.iou_mode == 0)
                and not self.single_frame and self.device.type == "cuda")

    def _plan_guard(self, flat, guard):
        """Tables of the frame-order guard (stage_iou_guard)."""
        if not self.guard_active():
            return
        lens = [int(np.diff(np.asarray(flat[s + "_frame_off"])).max())
                if len(flat[s + "_frame_off"]) > 1 else 0 for s in ("dt", "gt")]
        self.max_frames = lens
        # reordering bound of taoamd_track_iou_near (include/tao_amodal_hip.h)
        self.near_ulp = int(min(8 * (lens[0] + lens[1]) + 8, 2 ** 31 - 1))
        tl_id = np.ascontiguousarray(flat.tl_image_id, dtype=np.int64)
        ids_ok = len(tl_id) == 0 or (int(tl_id.min()) >= 0
                                     and int(tl_id.max()) < 2 ** 61 - 1)
        if guard == "device" and ids_ok:
            self.guard_on_device = True
            dev = self.device
            self.t["cell_unit"] = torch.from_numpy(
                np.ascontiguousarray(flat.cell_unit, dtype=np.int32)).to(dev)
            self.t["tl_vid_start"] = torch.from_numpy(
                np.ascontiguousarray(flat.tl_vid_start, dtype=np.int64)).to(dev)
            self.t["tl_image_id"] = torch.from_numpy(tl_id).to(dev)
        else:
            self.guard_flat = flat

    def input_bytes(self):
        return sum(v.numel() * v.element_size() for v in self.t.values()
                   if v is not None)


class Workspace:
    """Output and scratch buffers of one evaluator pass, allocated once."""

    def __init__(self, dp, detail=False, dt_rng_table=False, keep_order=False):
        lib = _lib.load()
        dev = dp.device
        u8 = torch.uint8
        # rows left in cell order and gathered by the sweep (run_forked) where
        # that is the faster form; the per-detection views want the rows sorted
        self.gather = not detail and gathers_rows(dp)

        def buf(nbytes):
            return torch.empty(max(int(nbytes), 256), dtype=u8, device=dev)
        self.gt_rng = torch.empty(max(dp.n_gt, 1), dtype=torch.int32, device=dev)
        # (image level: the match derives a detection's range mask from its
        # flags -- no table unless the caller wants to look at it)
        self.dt_rng = None if dp.kind == "lvis" and not (detail or dt_rng_table) \
            else torch.empty(max(dp.n_dt, 1), dtype=torch.int32, device=dev)
        self.num_gt = torch.empty((dp.n_cat, dp.n_rng), dtype=torch.int32,
                                  device=dev)
        # dst[i] = the place of detection i's row in `rows`.  Scatter form: its
        # sorted place, stored by the sort (the match writes the row there);
        # order[] = its inverse is derived on demand (the `order` property)
        # unless a caller wants the sort to store it: 86 MB of stores less per
        # pass at 21 M detections.  Gathered form: the sort stores order[] and
        # nothing else, the rows stay where the detections are and dst[] is the
        # identity, written once (dst_identity: it still is).
        self.order_buf = torch.empty(max(dp.n_dt, 1), dtype=torch.int32, device=dev) \
            if (detail or keep_order or self.gather) else None
        self._n_dt = dp.n_dt
        self.dst = torch.empty(max(dp.n_dt, 1), dtype=torch.int32, device=dev)
        self.dst_identity = False
        self.cell_order = False           # the last match left its rows in cell order
        self.sort_bytes = max(lib.taoamd_sort_workspace(dp.n_dt),
                              lib.taoamd_sort_segments_workspace(dp.n_dt),
                              lib.taoamd_sort_sampled_workspace(
                                  dp.n_dt, dp.ss_sizes[3], int(dp.ss_merge)))
        self.sort_ws = buf(self.sort_bytes)
        # rows of (matched, ignored) pairs, one pair per 64 combos: the match
        # stores a pair with one 16-byte store and the sweep loads it with one
        # load (the C ABI sees two tables, the second one word behind the first)
        # (rows / matched / ignored are read through the properties below: a
        # compact pass leaves most rows as 4-byte words)
        self._rows = torch.empty((max(dp.n_dt, 1), dp.n_words, 2),
                                 dtype=torch.int64, device=dev)
        self._matched, self._ignored = self._rows[..., 0], self._rows[..., 1]
        # gathered form: one 4-byte word per detection, in cell order, where the
        # row is a function of 18 bits (taoamd_match_compact); rows_pending: the
        # last match stored that form and `rows` has not been expanded from it
        self.compact_buf = torch.empty(max(dp.n_dt, 1), dtype=torch.int32, device=dev) \
            if self.gather else None
        self.rows_pending = False
        self.rows_expanded = 0            # expansions so far (taoamd_expand_rows)
        self._dp = dp
        self.acc_bytes = lib.taoamd_accumulate_workspace(dp.n_dt, dp.n_cat,
                                                         dp.n_rng)
        self.acc_ws = buf(self.acc_bytes)
        # the chunk table of the sweep depends on cat_off alone: built once here,
        # one launch less on the chain of every pass
        self.acc_prepared = None          # (max_segment hint, plan kind) it was built for
        self.sweep_recovered = 0          # passes swept again after a look-back gave up
        if torch.device(dev).type == "cuda":
            prepare_sweep(dp, self)
        self.precision = torch.empty((N_THR, N_REC, dp.n_cat, dp.n_rng),
                                     dtype=torch.float64, device=dev)
        self.recall = torch.empty((N_THR, dp.n_cat, dp.n_rng),
                                  dtype=torch.float64, device=dev)
        self.iou = None
        self.pair_frames = None
        if dp.kind == "tao":
            self.iou = torch.empty(max(dp.n_iou, 1), dtype=torch.float64,
                                   device=dev)
            self.pair_frames = torch.zeros(1, dtype=torch.int64, device=dev)
            self.near_count = torch.zeros(1, dtype=torch.int32, device=dev)
            self.guarded_pairs = 0
            # every pair can be listed: the list never overflows, so no pass
            # has to look at the count on the host
            self.near_cap = int(min(max(dp.n_iou, 1), 2 ** 31 - 1)) \
                if dp.guard_active() else 1
            self.near_list = torch.empty(self.near_cap, dtype=torch.int64, device=dev)
            if dp.guard_on_device:
                self.guard_table = int(lib.taoamd_track_iou_setorder_table(
                    *dp.max_frames))
                workers = GUARD_SCRATCH_BYTES // (12 * self.guard_table)
                workers = int(min(max(workers // 64 * 64, 64), 4096))
                self.guard_slots = workers * 3 * self.guard_table
                self.guard_scratch = torch.empty(self.guard_slots, dtype=torch.int32,
                                                 device=dev)
                self.guard_status = torch.zeros(1, dtype=torch.int32, device=dev)
        elif dp.mask_iou:
            self.iou = torch.empty(max(dp.n_iou, 1), dtype=torch.float64,
                                   device=dev)
        if dp.mask_iou:
            ws_bytes = lib.taoamd_rle_iou_workspace if dp.kind == "lvis" else \
                lib.taoamd_track_mask_iou_workspace
            self.rle_bytes = ws_bytes(dp.rle_rows["dt"], dp.rle_total["dt"],
                                      dp.rle_rows["gt"], dp.rle_total["gt"])
            self.rle_ws = buf(self.rle_bytes)
        self.match_gt = None
        self.ious_out = None
        if detail:
            self.match_gt = torch.empty((max(dp.n_dt, 1), dp.n_rng * N_THR),
                                        dtype=torch.int32, device=dev)
            if dp.kind == "lvis":
                self.ious_out = torch.empty(max(dp.n_iou, 1),
                                            dtype=torch.float64, device=dev)
        # the on-request analyses: allocated by their first call
        self.declare_products()
        self.pairs_counted = False        # stage_track_iou counted the pairs' common frames

    # What the on-request stages keep with the workspace (_buffer, _workspace)
    # or leave as their last result: None until a first call.  stage_scores,
    # the error breakdown, its impact and its confusion; *_order: the order[]
    # of the last call, conf_n: the entries of the last stage_confusion.
    ANALYSIS_PRODUCTS = (
        "score_ws", "score_bytes", "scores", "score_order",
        "err_ws", "err_bytes", "err_match_gt", "err_dt_counts", "err_gt_counts", "err_dt_type",
        "err_link_same", "err_link_other", "err_held",
        "imp_ws", "imp_bytes", "imp_precision", "imp_num_gt", "imp_order",
        "conf_ws", "conf_bytes", "conf_off", "conf_gt_cat", "conf_counts", "conf_n")

    # The track analyses.
    # ident_share holds the LAST run of taoamd_track_identity_share, whichever
    # stage asked for it (_identity_share): the shares at valid["share"], which
    # need not be the threshold of ident_keep / ident_gt / ident_dt /
    # ident_cat_counts (valid["identity"]).  The at_* are the thresholded
    # identity's own (stage_track_identity_at); occ_n, clear_n: the episodes /
    # candidates the last call read.
    TRACK_PRODUCTS = (
        "assoc_ws", "assoc_bytes", "assoc_follow", "assoc_gt", "assoc_cat_counts",
        "assoc_vis_counts", "assoc_best", "assoc_best_iou", "assoc_vis_rng",
        "occ_ws", "occ_bytes", "occ_gt", "occ_off", "occ_counts", "occ_episodes", "occ_n",
        "ident_ws", "ident_bytes", "ident_status", "ident_share", "ident_cat_counts", "ident_gt",
        "ident_dt", "ident_keep",
        "at_ws", "at_bytes", "at_status", "at_pass", "at_thr", "at_cat_counts", "at_dt", "at_gt",
        "at_keep",
        "hota_ws", "hota_bytes", "hota_status", "hota_pot", "hota_mc", "hota_lc", "hota_match",
        "hota_match_iou", "hota_tp", "hota_loc", "hota_ass",
        "clear_ws", "clear_bytes", "clear_status", "clear_off", "clear_step", "clear_cand",
        "clear_row", "clear_q", "clear_iou", "clear_n", "clear_match", "clear_match_iou",
        "clear_sw", "clear_gt", "clear_cat_counts", "clear_vis_counts")

    def declare_products(self):
        for name in self.ANALYSIS_PRODUCTS + self.TRACK_PRODUCTS:
            setattr(self, name, None)
        # product -> the key it is valid for (_valid, _producing): "followers"
        # (assoc_best and kin), "share" (ident_share), "identity" (ident_keep,
        # ident_gt, ident_dt, ident_cat_counts), each at its frame_thr; "match
        # indices" (err_match_gt holds those of a completed match); and a
        # stage's own buffers ("<stage> buffers": _stage_buffers) at their sizes
        self.valid = {}

    declare_track_products = declare_products     # (the name from before it set both tuples)


def _order_of(ws):
    """order[p] = detection at sorted place p: stored by the sort when the
    workspace asked for it, else the inverse of dst[] (of the last pass)."""
    if ws.order_buf is not None:
        return ws.order_buf
    n = ws._n_dt
    out = torch.empty(max(n, 1), dtype=torch.int32, device=ws.dst.device)
    if n:
        out[ws.dst[:n].long()] = torch.arange(n, dtype=torch.int32, device=ws.dst.device)
    return out


Workspace.order = property(_order_of)


def expand_rows(ws):
    """The full (matched, ignored) rows of the last pass: after a compact pass
    (stage_match on a gathering workspace) they are expanded from the 4-byte
    words on the current stream, once, until the next such pass."""
    if ws.rows_pending:
        dp = ws._dp
        with torch.cuda.device(dp.device):
            _lib.check(_lib.load().taoamd_expand_rows(
                dp.n_dt, dp.n_rng, _ptr(ws.compact_buf), _ptr(ws._rows), _stream()),
                "taoamd_expand_rows")
        ws.rows_pending = False
        ws.rows_expanded += 1
    return ws


Workspace.rows = property(lambda ws: expand_rows(ws)._rows)
Workspace.matched = property(lambda ws: expand_rows(ws)._matched)
Workspace.ignored = property(lambda ws: expand_rows(ws)._ignored)


def stage_ranges(dp, ws):
    lib, t, s = _lib.load(), dp.t, _stream()
    if dp.kind == "lvis":
        _lib.check(lib.taoamd_lvis_ranges(
            dp.n_gt, _ptr(t["gt_vis"]), _ptr(t["gt_flags"]), _ptr(t["gt_cat"]),
            _ptr(t["gt_cat_off"]) if dp.grouped else None,
            dp.n_dt, _ptr(t["dt_flags"]), dp.n_cat, _ptr(ws.gt_rng),
            _ptr(ws.dt_rng), _ptr(ws.num_gt), s), "taoamd_lvis_ranges")
    else:
        _lib.check(lib.taoamd_tao_ranges(
            dp.n_gt, _ptr(t["gt_area"]), _ptr(t["gt_len"]), _ptr(t["gt_nhp"]),
            _ptr(t["gt_flags"]), _ptr(t["gt_cat"]),
            _ptr(t["gt_cat_off"]) if dp.grouped else None, dp.n_dt,
            _ptr(t["dt_area"]), _ptr(t["dt_len"]), _ptr(t["dt_flags"]),
            dp.n_cat, _ptr(ws.gt_rng), _ptr(ws.dt_rng), _ptr(ws.num_gt), s),
            "taoamd_tao_ranges")


# Which segment sort a pass takes.  The sample sort (taoamd_sort_sampled: one
# scatter pass + one register sort per bucket) wins where categories span many
# LDS tiles -- 2000 videos, 21 M detections: 0.62 against 0.79 ms -- but is four
# dependent launches; below SORT_SAMPLED_MIN detections the tile sort + one
# rank-merge pass (taoamd_sort_segments) is the shorter chain.  (Until the
# bucket sort's exchanges became DPP moves the threshold was 6 M -- Config 2,
# 2.1 M detections: 107 against 130 us; since then the sample sort takes 80 us
# there against 102, and 67 against 77 at the 3 M rows of the stress stand-in.)
# _SORT_FORCE "sampled" / "segments" forces one (the tests' way onto the sample
# sort with small inputs).
SORT_SAMPLED_MIN = 1_500_000
_SORT_FORCE = ""


def sort_is_sampled(dp):
    if _SORT_FORCE in ("sampled", "segments"):
        return _SORT_FORCE == "sampled"
    return dp.n_dt >= SORT_SAMPLED_MIN


# Image level, Overlap's chain: where the match leaves its rows (run_forked).
# Cell order + gathering sweep where gathers_rows() says so, the scatter form
# everywhere else.  Measured on one MI355X at 21.4 M rows, three runs each:
# scatter form 1.356-1.361 ms a step, cell order 1.290-1.304 (the sort
# stores no dst[], the match reads none, stores whole-wavefront runs and runs
# beside the sort; the one-pass sweep's gathered loader pays part of it back).
# The round-2 form of the same idea -- generic loader, unprepared plan, the slow
# match kernel -- was and is a loss: 1.364-1.371 ms.

def gathers_rows(dp):
    """Whether Overlap's image-level chain leaves the match's rows in cell
    order on this problem: box IoU, grouped plan, the sample sort (it can store
    order[] alone) and the one-pass sweep (it reads every row once: the 6 M-row
    rule of taoamd_accumulate_plan_kind) on one GPU."""
    return (dp.kind == "lvis" and not dp.mask_iou and dp.grouped and dp.n_dt > 0
            and dp.device.type == "cuda" and sort_is_sampled(dp)
            and _plan_key(dp)[1] in (2, 3))


def stage_sort(dp, ws, order_only=False):
    lib, t, s = _lib.load(), dp.t, _stream()
    if not order_only:
        ws.dst_identity = False
    if dp.grouped and dp.n_dt and sort_is_sampled(dp):
        nc, ns, nt, nb = dp.ss_sizes
        _lib.check(lib.taoamd_sort_sampled(
            dp.n_dt, dp.n_cat, _ptr(t["cat_off"]), _ptr(t["tile_off"]), dp.n_tiles,
            dp.max_segment, _ptr(t["dt_score"]), nc, _ptr(t["ss_chunks"]), ns,
            _ptr(t["ss_split"]), nt, _ptr(t["ss_stile"]), nb, _ptr(t["ss_bucket"]),
            _ptr(ws.order_buf), None if order_only else _ptr(ws.dst), _ptr(ws.sort_ws),
            ws.sort_bytes, s),
            "taoamd_sort_sampled")
        return
    if dp.grouped:
        _lib.check(lib.taoamd_sort_segments(
            dp.n_dt, dp.n_cat, _ptr(t["cat_off"]), _ptr(t["tile_off"]),
            dp.n_tiles, dp.max_segment, _ptr(t["dt_cat"]), _ptr(t["dt_score"]),
            _ptr(ws.order_buf), _ptr(ws.dst), _ptr(ws.sort_ws), ws.sort_bytes, s),
            "taoamd_sort_segments")
        return
    _lib.check(lib.taoamd_sort_by_cat_score(
        dp.n_dt, _ptr(t["dt_cat"]), _ptr(t["dt_score"]), _ptr(ws.order_buf),
        _ptr(ws.dst), _ptr(ws.sort_ws), ws.sort_bytes, s),
        "taoamd_sort_by_cat_score")


def stage_mask_iou(dp, ws):
    """IoU of the run-length masks of every cell (iou_type="segm")."""
    if not dp.mask_iou or dp.n_iou == 0:
        return
    lib, t, s = _lib.load(), dp.t, _stream()
    _lib.check(lib.taoamd_rle_iou(
        dp.n_cells, _ptr(t["cell_dt_off"]), _ptr(t["cell_gt_off"]),
        _ptr(t["cell_iou_off"]), dp.n_dt, dp.rle_total["dt"],
        _ptr(t["dt_rle_off"]), _ptr(t["dt_rle_runs"]), _ptr(t["dt_rle_hw"]),
        _ptr(t["dt_rle_bb"]), dp.n_gt, dp.rle_total["gt"],
        _ptr(t["gt_rle_off"]), _ptr(t["gt_rle_runs"]), _ptr(t["gt_rle_hw"]),
        _ptr(t["gt_rle_bb"]), _ptr(ws.iou), _ptr(ws.rle_ws), ws.rle_bytes, s),
        "taoamd_rle_iou")


def stage_track_mask_iou(dp, ws):
    """3D IoU of the mask tracks of every cell (TaoEval iou_type="segm"); the
    count of shared (pair, frame) items goes to ws.pair_frames."""
    lib, t, s = _lib.load(), dp.t, _stream()
    _lib.check(lib.taoamd_track_mask_iou(
        dp.n_cells, _ptr(t["cell_dt_off"]), _ptr(t["cell_gt_off"]),
        _ptr(t["cell_iou_off"]), dp.n_iou, _ptr(t["dt_frame_off"]),
        _ptr(t["dt_frame_pos"]), dp.rle_rows["dt"], dp.rle_total["dt"],
        _ptr(t["dt_rle_off"]), _ptr(t["dt_rle_runs"]), _ptr(t["dt_rle_hw"]),
        _ptr(t["gt_frame_off"]), _ptr(t["gt_frame_pos"]), dp.rle_rows["gt"],
        dp.rle_total["gt"], _ptr(t["gt_rle_off"]), _ptr(t["gt_rle_runs"]),
        _ptr(t["gt_rle_hw"]), dp.iou_mode, _ptr(ws.iou), _ptr(ws.pair_frames), _ptr(ws.rle_ws),
        ws.rle_bytes, s), "taoamd_track_mask_iou")


def stage_track_iou(dp, ws):
    if dp.kind == "lvis":
        return stage_mask_iou(dp, ws)        # the image level's pre-match IoU
    if dp.kind != "tao" or dp.n_iou == 0:
        return
    if dp.mask_iou:
        return stage_track_mask_iou(dp, ws)
    lib, t, s = _lib.load(), dp.t, _stream()
    if dp.single_frame:
        _lib.check(lib.taoamd_track_iou_single(
            dp.n_dt, _ptr(t["dt_group"]), _ptr(t["cell_iou_off"]),
            _ptr(t["dt_frame_pos"]), _ptr(t["dt_frame_box"]), _ptr(t["gt_frame_pos"]),
            _ptr(t["gt_frame_box"]), dp.iou_mode, _ptr(ws.iou), _ptr(ws.pair_frames), s),
            "taoamd_track_iou_single")
        return
    if t["tasks"] is not None:
        # the pairs' common frames (pair_frames: the unit the throughput is
        # quoted in) are a constant of the problem: counted by the first pass
        # over a workspace, which later passes leave as it is -- the 3D IoU's
        # arithmetic needs no frame masks, the kernel is 5 % shorter without them
        counted = ws.pairs_counted and dp.iou_mode == 0
        _lib.check(lib.taoamd_track_iou_planned(
            dp.n_tasks, _ptr(t["tasks"]), _ptr(t["task_rows"]),
            _ptr(t["task_pairs"]), _ptr(t["task_out"]), _ptr(t["frames"]),
            _ptr(t["task_base"]), _ptr(t["trk_meta"]), dp.iou_mode, _ptr(ws.iou),
            None if counted else _ptr(ws.pair_frames), int(t["zero_out"].numel()),
            _ptr(t["zero_out"]), s), "taoamd_track_iou_planned")
        ws.pairs_counted = True
        return
    _lib.check(lib.taoamd_track_iou(
        dp.n_cells, _ptr(t["cell_dt_off"]), _ptr(t["cell_gt_off"]),
        _ptr(t["cell_iou_off"]), dp.n_iou, _ptr(t["dt_frame_off"]),
        _ptr(t["dt_frame_pos"]), _ptr(t["dt_frame_box"]),
        _ptr(t["gt_frame_off"]), _ptr(t["gt_frame_pos"]),
        _ptr(t["gt_frame_box"]), dp.iou_mode, _ptr(ws.iou),
        _ptr(ws.pair_frames), s), "taoamd_track_iou")


GUARD_SCRATCH_BYTES = 64 << 20    # set tables of the device-side guard's threads


def stage_iou_guard(dp, ws):
    """The frame-order guard, all on the device: list the track pairs whose
    IoU a reordering of the frame sums could move across a comparison of the
    match (taoamd_track_iou_near, within dp.near_ulp of a threshold or of a
    rival), then recompute exactly those in the reference's CPython set order
    (taoamd_track_iou_setorder) and patch the IoU matrix -- asynchronous, no
    host round trip.  Nothing to do for integer boxes under the 3D IoU (exact
    sums) and for the count-based imagenetvid IoU."""
    if not dp.guard_active():
        return
    lib, t, s = _lib.load(), dp.t, _stream()
    _lib.check(lib.taoamd_track_iou_near(
        dp.n_cells, _ptr(t["cell_gt_off"]), _ptr(t["cell_iou_off"]), dp.n_iou,
        _ptr(ws.iou), dp.near_ulp, ws.near_cap, _ptr(ws.near_count),
        _ptr(ws.near_list), s), "taoamd_track_iou_near")
    if not dp.guard_on_device:
        return
    _lib.check(lib.taoamd_track_iou_setorder(
        dp.n_cells, _ptr(t["cell_dt_off"]), _ptr(t["cell_gt_off"]),
        _ptr(t["cell_iou_off"]), _ptr(t["cell_unit"]), _ptr(t["tl_vid_start"]),
        _ptr(t["tl_image_id"]), _ptr(t["dt_frame_off"]), _ptr(t["dt_frame_pos"]),
        _ptr(t["dt_frame_box"]), _ptr(t["gt_frame_off"]), _ptr(t["gt_frame_pos"]),
        _ptr(t["gt_frame_box"]), dp.iou_mode, _ptr(ws.near_count), ws.near_cap,
        _ptr(ws.near_list), _ptr(ws.iou), _ptr(ws.guard_scratch), ws.guard_slots,
        ws.guard_table, _ptr(ws.guard_status), s), "taoamd_track_iou_setorder")


def apply_iou_guard(dp, ws, flat=None):
    """Host half of the guard, for problems the device cannot recompute (an
    image id outside [0, 2^61 - 1): hash(id) != id) or that asked for it
    (DeviceProblem(guard="host"), the tests' cross-check): the listed pairs
    are recomputed with Python's own sets and patched into the IoU matrix
    before the match.  Returns the number of guarded pairs (synchronises)."""
    if not dp.guard_active() or dp.guard_on_device:
        return 0
    flat = flat if flat is not None else dp.guard_flat
    n = int(ws.near_count.item())
    if n == 0:
        return 0
    pairs = ws.near_list[:n].cpu().numpy()
    vals = set_order_iou(flat, pairs, dp.iou_mode)
    ws.iou[torch.from_numpy(pairs).to(dp.device)] = torch.from_numpy(vals).to(dp.device)
    return n


def _plan_key(dp):
    return (dp.acc_hint, int(_lib.load().taoamd_accumulate_plan_kind(
        dp.n_dt, dp.n_rng, dp.acc_hint)))


def prepare_sweep(dp, ws):
    """(Re)build the sweep's plan in the workspace (taoamd_accumulate_prepare):
    the table that cuts the categories into chunks / super-chunks under the
    current sweep mode."""
    with torch.cuda.device(dp.device):
        _lib.check(_lib.load().taoamd_accumulate_prepare(
            dp.n_dt, dp.n_cat, dp.n_rng, _ptr(dp.t["cat_off"]), dp.acc_hint,
            _ptr(ws.acc_ws), ws.acc_bytes, _stream()), "taoamd_accumulate_prepare")
    ws.acc_prepared = _plan_key(dp)


def sweep_flag(acc_ws, device):
    """The one-pass sweep's error flag of a workspace (taoamd_accumulate_error;
    synchronises with the current stream)."""
    import ctypes as C
    flag = C.c_int32(0)
    with torch.cuda.device(device):
        _lib.check(_lib.load().taoamd_accumulate_error(
            _ptr(acc_ws), _stream(), C.addressof(flag)), "taoamd_accumulate_error")
    return int(flag.value)


def sweep_ok(dp, ws):
    """Check the last pass on this workspace for the one-pass sweep's error flag
    (a look-back between workgroups gave up waiting; synchronises).  Such a
    pass is swept AGAIN with the chunked kernels -- its rows are still in the
    workspace -- so precision / recall are the right tables when this returns;
    the plan is rebuilt for the passes to come.  Returns True if it had to."""
    if dp.device.type != "cuda" or not sweep_flag(ws.acc_ws, dp.device):
        return False
    import logging
    logging.getLogger("tao_amodal_amd").warning(
        "the one-pass sweep's look-back between workgroups timed out (a busy or "
        "shared GPU?): this pass is swept again with the chunked kernels")
    lib, t = _lib.load(), dp.t
    with torch.cuda.device(dp.device):
        if ws.cell_order:
            # (the rows are where the match left them, order[] where the sort did)
            _lib.check(lib.taoamd_accumulate_by_order_chunked(
                dp.n_dt, dp.n_cat, dp.n_rng, _ptr(t["cat_off"]), _ptr(ws.order),
                _ptr(ws.matched), _ptr(ws.ignored), _ptr(ws.num_gt), dp.acc_hint,
                _ptr(ws.precision), _ptr(ws.recall), _ptr(ws.acc_ws), ws.acc_bytes,
                _stream()), "taoamd_accumulate_by_order_chunked")
        else:
            _lib.check(lib.taoamd_accumulate_chunked(
                dp.n_dt, dp.n_cat, dp.n_rng, _ptr(t["cat_off"]), _ptr(ws.matched),
                _ptr(ws.ignored), _ptr(ws.num_gt), dp.acc_hint, _ptr(ws.precision),
                _ptr(ws.recall), _ptr(ws.acc_ws), ws.acc_bytes, _stream()),
                "taoamd_accumulate_chunked")
    prepare_sweep(dp, ws)
    torch.cuda.synchronize(dp.device)
    ws.sweep_recovered += 1
    return True


def guarded_pairs(dp, ws, check_sweep=True):
    """Pairs the last pass listed and recomputed (synchronises).  Also the
    place where a pass is checked for the sweep's error flag (and swept again
    if it is set: sweep_ok; the multi-GPU plans check the workspace they swept
    on themselves, collectively: dist.ShardedEval.check)."""
    if check_sweep:
        sweep_ok(dp, ws)
    if not dp.guard_active():
        return 0
    if dp.guard_on_device and int(ws.guard_status.item()):
        raise _lib.TaoAmdError("frame-order guard: a track pair outgrew the set "
                               "tables sized for the longest tracks")
    n = int(ws.near_count.item())
    if n > max(dp.n_iou // 8, 1024):
        # every listed pair is recomputed serially by one thread (the CPython
        # set emulation): a large share of the pairs -- avg_iou on integer
        # boxes with many exact ties, duplicated tracks -- turns a 0.3 ms pass
        # into a much longer one without changing any result; say so
        import logging
        logging.getLogger("tao_amodal_amd").warning(
            "frame-order guard: %d of %d track pairs were recomputed in the "
            "reference's frame order (slow path)", n, dp.n_iou)
    return n


def _fmax(a, b):
    """Python's max(a, b) on numbers; where one is a NaN, the other (C's fmax:
    the rule of the kernels on boxes that are any double)."""
    return b if (b > a or a != a) else a


def _fmin(a, b):
    return b if (b < a or a != a) else a


def _pos(w):
    """Python's max(w, 0), and 0 for a NaN (C's ``w > 0 ? w : 0``)."""
    return 0 if (0 > w or w != w) else w


def set_order_iou(flat, pairs, mode=0):
    """3D IoU (mode 0) / average IoU (mode 1) of the listed pairs exactly as
    the reference computes them: {image id: box} maps in annotation order, the
    frames visited in the iteration order of
    ``set(gt.keys()) | set(dt.keys())`` (T/eval.py:73-117).  On a NaN
    coordinate the per-frame terms follow C (_fmax, _fmin, _pos), as every
    kernel does: the same bits as Python's max / min on everything else."""
    ioff = np.asarray(flat.cell_iou_off)
    d_off, g_off = np.asarray(flat.cell_dt_off), np.asarray(flat.cell_gt_off)
    tl_id, tl_start = np.asarray(flat.tl_image_id), np.asarray(flat.tl_vid_start)
    unit = np.asarray(flat.cell_unit)
    fr = {}
    for side in ("dt", "gt"):
        fr[side] = (np.asarray(flat[side + "_frame_off"]),
                    np.asarray(flat[side + "_frame_pos"]),
                    np.asarray(flat[side + "_frame_box"]))
    cache = {}

    def track_map(side, t, v):
        key = (side, t)
        if key not in cache:
            off, pos, box = fr[side]
            a, b = int(off[t]), int(off[t + 1])
            ids = tl_id[tl_start[v] + pos[a:b]].tolist()
            cache[key] = dict(zip(ids, np.asarray(box[a:b]).tolist()))
        return cache[key]
    out = np.zeros(len(pairs))
    cells = np.searchsorted(ioff, pairs, "right") - 1
    for k, (p, c) in enumerate(zip(pairs.tolist(), cells.tolist())):
        G = int(g_off[c + 1] - g_off[c])
        local = p - int(ioff[c])
        v = int(unit[c])
        dmap = track_map("dt", int(d_off[c]) + local // G, v)
        gmap = track_map("gt", int(g_off[c]) + local % G, v)
        i = u = 0
        ious = []
        for im in set(gmap.keys()) | set(dmap.keys()):
            g, d = gmap.get(im), dmap.get(im)
            if d and g:
                w = _pos(_fmin(d[0] + d[2], g[0] + g[2]) - _fmax(d[0], g[0]))
                h = _pos(_fmin(d[1] + d[3], g[1] + g[3]) - _fmax(d[1], g[1]))
                i_ = w * h
                u_ = d[2] * d[3] + g[2] * g[3] - i_
                i += i_
                u += u_
                ious.append(i_ / u_ if u_ > 0 else 0)
            elif g:
                u += g[2] * g[3]
                ious.append(0)
            elif d:
                u += d[2] * d[3]
                ious.append(0)
        out[k] = (i / u if u > 0 else 0) if mode == 0 else float(np.mean(ious))
    return out


def stage_match(dp, ws, scatter=True, groups=None, singles=None, match_gt=None):
    """`groups` / `singles`: (device table, first, count) -- a slice of a
    launch plan instead of the problem's whole plan (the phases of the
    multi-GPU exchange, dist.ShardedEval).  `match_gt`: a table for the in-cell
    match indices of this one call, where the workspace keeps none; handed the
    workspace's own error_match_gt(), the call produces "match indices"."""
    if match_gt is not None and match_gt is ws.err_match_gt:
        with _producing(ws, "match indices", ()):
            return _match(dp, ws, scatter, groups, singles, match_gt)
    return _match(dp, ws, scatter, groups, singles, match_gt)


def _match(dp, ws, scatter, groups, singles, match_gt):
    if dp.n_dt == 0:        # nothing was detected: every cell is GT-only
        return
    lib, t, s = _lib.load(), dp.t, _stream()
    g_ptr, n_g = _ptr(t["groups"]), dp.n_groups
    s_ptr, n_s = _ptr(t["singles"]), dp.n_singles
    if groups is not None:
        g_ptr, n_g = groups[0].data_ptr() + 16 * groups[1], groups[2]
        s_ptr, n_s = singles[0].data_ptr() + 4 * singles[1], singles[2]
        if n_g == 0 and n_s == 0:
            return
    fused = dp.kind == "lvis" and not dp.mask_iou
    if groups is None:
        ws.cell_order = not scatter
    # the compact form exactly where the workspace gathers: the whole plan, rows
    # in cell order, no per-detection tables asked for
    if (ws.gather and not scatter and groups is None and match_gt is None
            and ws.match_gt is None and ws.ious_out is None):
        _lib.check(lib.taoamd_match_compact(
            dp.n_cells, _ptr(t["cell_dt_off"]), _ptr(t["cell_gt_off"]), dp.max_g,
            _ptr(t["dt_box"]), _ptr(t["gt_box"]), dp.n_rng, _ptr(ws.gt_rng),
            _ptr(t["gt_flags"]), _ptr(t["dt_flags"]), _ptr(ws._rows), _ptr(ws.compact_buf),
            _ptr(t["dt_group"]), _ptr(t["dt_meta"]), g_ptr, n_g, s_ptr, n_s, s),
            "taoamd_match_compact")
        ws.rows_pending = True
        return
    if groups is None:
        ws.rows_pending = False       # (every row is stored in full)
    _lib.check(lib.taoamd_match(
        dp.n_cells, _ptr(t["cell_dt_off"]), _ptr(t["cell_gt_off"]),
        _ptr(t["cell_iou_off"]), dp.max_g,
        _ptr(t["dt_box"]) if fused else None,
        _ptr(t["gt_box"]) if fused else None,
        None if fused else _ptr(ws.iou), dp.n_rng, _ptr(ws.gt_rng),
        None if dp.kind == "lvis" else _ptr(ws.dt_rng),   # (image level: from the flags)
        _ptr(t["gt_flags"]), _ptr(t["dt_flags"]),
        _ptr(ws.dst) if scatter else None, 0, _ptr(ws.matched),
        _ptr(ws.ignored), _ptr(ws.match_gt if match_gt is None else match_gt),
        _ptr(ws.ious_out),
        _ptr(t["dt_group"]), _ptr(t["dt_meta"]), g_ptr, n_g,
        s_ptr, n_s, s), "taoamd_match")


def stage_accumulate_by_order(dp, ws):
    """The sweep over rows the match left in cell order (stage_match(scatter=
    False)): gathered through the sort's order[] by the first sweep."""
    lib, t, s = _lib.load(), dp.t, _stream()
    key = _plan_key(dp)
    if ws.rows_pending and key[1] in (2, 3):
        # (the one-pass sweep reads the 4-byte words; `rows` stays unexpanded)
        _lib.check(lib.taoamd_accumulate_by_order_compact(
            dp.n_dt, dp.n_cat, dp.n_rng, _ptr(t["cat_off"]), _ptr(ws.order),
            _ptr(ws.compact_buf), _ptr(ws._rows), _ptr(ws.num_gt), dp.acc_hint,
            _ptr(ws.precision), _ptr(ws.recall), _ptr(ws.acc_ws), ws.acc_bytes,
            int(ws.acc_prepared == key), s), "taoamd_accumulate_by_order_compact")
        return
    fn = lib.taoamd_accumulate_by_order_prepared if ws.acc_prepared == key \
        else lib.taoamd_accumulate_by_order
    _lib.check(fn(
        dp.n_dt, dp.n_cat, dp.n_rng, _ptr(t["cat_off"]), _ptr(ws.order),
        _ptr(ws.matched), _ptr(ws.ignored), _ptr(ws.num_gt), dp.acc_hint,
        _ptr(ws.precision), _ptr(ws.recall), _ptr(ws.acc_ws), ws.acc_bytes, s),
        "taoamd_accumulate_by_order")


def stage_accumulate(dp, ws):
    lib, t, s = _lib.load(), dp.t, _stream()
    # (a plan built under another sweep mode or hint does not serve this pass)
    fn = lib.taoamd_accumulate_prepared if ws.acc_prepared == _plan_key(dp) \
        else lib.taoamd_accumulate
    _lib.check(fn(
        dp.n_dt, dp.n_cat, dp.n_rng, _ptr(t["cat_off"]), _ptr(ws.matched),
        _ptr(ws.ignored), _ptr(ws.num_gt), dp.acc_hint, _ptr(ws.precision),
        _ptr(ws.recall), _ptr(ws.acc_ws), ws.acc_bytes, s),
        "taoamd_accumulate")


def stage_scores(dp, ws):
    """eval["scores"] of the pass the workspace holds (after stage_accumulate):
    ws.scores[T, R, n_cat, n_rng] = the score of the row at which recall first
    reaches each recall threshold (taoamd_score_at_recall), under the calling
    thread's thresholds.  Its buffers are allocated on the first call: a
    workspace that is never asked pays nothing."""
    lib, t, s = _lib.load(), dp.t, _stream()
    _stage_buffers(
        ws, dp.device, "score", (), lambda: lib.taoamd_score_at_recall_workspace(
            dp.n_dt, dp.n_cat, dp.n_rng),
        lambda: (("scores", (N_THR, N_REC, dp.n_cat, dp.n_rng), torch.float64),))
    # the scores lie where the detections are; so do rows left in cell order,
    # rows scattered to their sorted places need order[] for the scores alone
    ws.score_order = ws.order        # (derived on demand: alive while the pass runs)
    order = _ptr(ws.score_order)
    _lib.check(lib.taoamd_score_at_recall(
        dp.n_dt, dp.n_cat, dp.n_rng, _ptr(t["cat_off"]), order if ws.cell_order else None,
        _ptr(ws.matched), _ptr(ws.ignored), _ptr(t["dt_score"]), order, _ptr(ws.num_gt),
        _ptr(ws.scores), _ptr(ws.score_ws), ws.score_bytes, s), "taoamd_score_at_recall")


def _rows_by_unit(unit, n_unit):
    """CSR of the rows of a table by the unit (image) they belong to, rows of a
    unit ascending: (off int32[n_unit + 1], rows int32[n])."""
    off = torch.zeros(n_unit + 1, dtype=torch.int32, device=unit.device)
    if unit.numel() == 0:
        return off, torch.zeros(1, dtype=torch.int32, device=unit.device)
    off[1:] = torch.cumsum(torch.bincount(unit, minlength=n_unit), 0)
    return off, torch.argsort(unit, stable=True).to(torch.int32)


def error_match_gt(dp, ws):
    """The table stage_error_types reads the match indices from where the
    workspace keeps none of its own: int32[n_dt, n_rng * 10], allocated on the
    first call and kept with the workspace (240 bytes a row: 5.1 GB at 21.4 M
    rows; `ws.err_match_gt = None` gives it back).  A caller that runs the match
    itself passes it as stage_match(match_gt=...) / run_guarded(match_gt=...):
    that match produces "match indices", the allocation alone does not."""
    if ws.err_match_gt is None:
        ws.valid.pop("match indices", None)       # (a new table holds none)
    return _buffer(ws, dp.device, "err_match_gt", (max(dp.n_dt, 1), dp.n_rng * N_THR),
                   torch.int32)


def _error_tabs(dp):
    """The breakdown's per-unit (image / video) row lists, built once per
    problem: dp.err_tabs = (units, gt_off, gt_rows, dt_off, dt_rows), the CSRs of
    _rows_by_unit; beside it dp.err_dt_gt0, the image level's column of every
    row's first ground truth."""
    if dp.err_tabs is None:
        t, dev = dp.t, dp.device
        cell_unit = torch.from_numpy(np.ascontiguousarray(dp.cell_unit_host, dtype=np.int64)
                                     ).to(dev)
        n_unit = int(dp.cell_unit_host.max()) + 1 if dp.n_cells else 0
        cells = torch.arange(dp.n_cells, dtype=torch.int64, device=dev)
        gt_cell = torch.repeat_interleave(
            cells, (t["cell_gt_off"][1:] - t["cell_gt_off"][:-1]).long())
        dt_cell = t["dt_cell"][:dp.n_dt].long()
        dp.err_tabs = (n_unit,) + _rows_by_unit(cell_unit[gt_cell], n_unit) \
            + _rows_by_unit(cell_unit[dt_cell], n_unit)
        if dp.kind == "lvis":
            dp.err_dt_gt0 = t["dt_group"][:, 0].contiguous()
    return dp.err_tabs


def _error_buffers(dp, ws, lib, per_detection, links):
    """The breakdown's buffers, each allocated where first asked for: the
    counts and the level's workspace, ws.err_dt_type with `per_detection`, the
    link tables and ws.err_held with `links`.  What a caller may give back by
    name (here the link tables) is under no key: asked for on every call."""
    sized = lib.taoamd_error_types_workspace if dp.kind == "lvis" else \
        lib.taoamd_track_error_types_workspace
    dev, shape, u8, i64 = dp.device, (max(dp.n_dt, 1), dp.n_rng), torch.uint8, torch.int64
    _stage_buffers(
        ws, dev, "err", (bool(per_detection), bool(links)),
        lambda: sized(dp.n_dt, dp.n_gt, dp.n_rng), lambda: (
            ("err_dt_counts", (dp.n_rng, dp.n_cat, 7), i64),
            ("err_gt_counts", (dp.n_rng, dp.n_cat, 3), i64))
        + ((("err_dt_type", shape, u8),) if per_detection else ())
        + ((("err_held", (dp.n_rng, max(dp.n_gt, 1)), u8),) if links else ()))
    if links:
        _buffer(ws, dev, "err_link_same", shape, torch.int32)
        _buffer(ws, dev, "err_link_other", shape, torch.int32)


def _impact_buffers(dp, ws, lib, name):
    """The buffers of the sweep of the nine variants through the entry point `name`."""
    sizes, fixes = (dp.n_cat, dp.n_rng), len(_lib.ERROR_FIXES)
    _workspace(ws, dp.device, "imp", getattr(lib, name + "_workspace")(dp.n_dt, dp.n_gt, *sizes))
    _buffer(ws, dp.device, "imp_precision", (fixes, N_REC) + sizes, torch.float64)
    _buffer(ws, dp.device, "imp_num_gt", (fixes,) + sizes, torch.int32)


def _confusion_buffers(dp, ws, lib):
    """The histogram's workspace and its row offsets; the entries: _confusion_entries."""
    _workspace(ws, dp.device, "conf",
               lib.taoamd_confusion_workspace(dp.n_dt, dp.n_gt, dp.n_cat, dp.n_rng))
    _buffer(ws, dp.device, "conf_off", dp.n_rng * dp.n_cat + 1, torch.int64)


def _confusion_entries(dp, ws, n):
    """ws.conf_n = n and room for n entries, regrown where a call finds more."""
    ws.conf_n = n
    _buffer(ws, dp.device, "conf_gt_cat", max(n, 1), torch.int32)
    _buffer(ws, dp.device, "conf_counts", (max(n, 1), 4), torch.int32)


def _error_match_gt(dp, ws):
    """The match indices the breakdown reads: the workspace's own table (detail
    mode), else error_match_gt(), filled by one more match unless the workspace
    holds "match indices": a completed match, this one or the caller's, wrote
    the table that is there."""
    if ws.match_gt is not None:
        return ws.match_gt
    if dp.n_dt and (ws.err_match_gt is None or not _valid(ws, "match indices", ())):
        with _producing(ws, "match indices", ()):
            stage_match(dp, ws, scatter=not ws.cell_order, match_gt=error_match_gt(dp, ws))
    return ws.err_match_gt


def _error_pass(dp, ws, slot, tb, kind, per_detection=False, links=False):
    """stage_error_types (`kind` "lvis") / stage_track_error_types ("tao"):
    `kind` is the level the caller's name promises, refused where the problem
    is of the other.  `links`: through the level's *_links entry point, which
    also fills ws.err_link_same, ws.err_link_other and ws.err_held."""
    track = kind == "tao"
    if dp.kind != kind or dp.mask_iou:
        raise _lib.TaoAmdError("the track-level error breakdown is the track level's, on boxes"
                               if track else "the error breakdown is the image level's, on boxes")
    if track and dp.iou_mode != 0:
        raise _lib.TaoAmdError("the track-level error breakdown is defined for the 3d_iou metric")
    if dp.cell_unit_host is None:
        raise _lib.TaoAmdError("the error breakdown needs the cells' %s (flat.cell_unit)"
                               % ("videos" if track else "images"))
    lib, t, s = _lib.load(), dp.t, _stream()
    n_unit, *lists = _error_tabs(dp)
    _error_buffers(dp, ws, lib, per_detection, links)
    match_gt = _error_match_gt(dp, ws)
    lists = tuple(_ptr(x) for x in lists)
    out = (_ptr(ws.err_dt_counts), _ptr(ws.err_gt_counts),
           _ptr(ws.err_dt_type) if per_detection else None)
    if kind == "lvis":
        name = "taoamd_error_types"
        args = (dp.n_dt, dp.n_gt, n_unit, dp.n_cat, dp.n_rng, int(slot), float(tb),
                _ptr(t["dt_cat"]), _ptr(t["dt_box"]), _ptr(t["dt_flags"]), _ptr(dp.err_dt_gt0),
                _ptr(match_gt), dp.n_rng * N_THR, _ptr(t["gt_cat"]), _ptr(t["gt_box"]),
                _ptr(ws.gt_rng)) + lists + out
    else:
        name = "taoamd_track_error_types"
        args = (dp.n_dt, dp.n_gt, dp.n_cells, dp.n_iou, n_unit, dp.n_cat, dp.n_rng, int(slot),
                float(tb), _ptr(t["dt_cat"]), _ptr(ws.dt_rng), _ptr(t["dt_group"]),
                _ptr(t["cell_iou_off"]), _ptr(ws.iou), _ptr(match_gt), dp.n_rng * N_THR,
                _ptr(t["gt_cat"]), _ptr(ws.gt_rng),
                _ptr(t["dt_frame_off"]), _ptr(t["dt_frame_pos"]), _ptr(t["dt_frame_box"]),
                _ptr(t["gt_frame_off"]), _ptr(t["gt_frame_pos"]), _ptr(t["gt_frame_box"])) \
            + lists + out + (None,)
    if links:
        name += "_links"
        args += (_ptr(ws.err_link_same), _ptr(ws.err_link_other), _ptr(ws.err_held))
    _lib.check(getattr(lib, name)(*args, _ptr(ws.err_ws), ws.err_bytes, s), name)


def _error_impact(dp, ws, slot, tb, kind):
    """stage_error_impact (`kind` "lvis") / stage_track_error_impact ("tao"): the
    level's links pass, then the sweep of the nine variants through the level's
    entry point -- the two share their signature."""
    _error_pass(dp, ws, slot, tb, kind, per_detection=True, links=True)
    lib, t = _lib.load(), dp.t
    name = "taoamd_error_impact" if kind == "lvis" else "taoamd_track_error_impact"
    _impact_buffers(dp, ws, lib, name)
    ws.imp_order = ws.order          # (derived on demand: alive while the pass runs)
    _lib.check(getattr(lib, name)(
        dp.n_dt, dp.n_gt, dp.n_cat, dp.n_rng, _ptr(t["cat_off"]), _ptr(ws.imp_order),
        _ptr(t["dt_score"]), _ptr(t["dt_cat"]), _ptr(ws.err_dt_type), _ptr(ws.err_link_same),
        _ptr(ws.err_link_other), _ptr(t["gt_cat"]), _ptr(ws.gt_rng), _ptr(ws.err_held),
        _ptr(ws.imp_precision), _ptr(ws.imp_num_gt), _ptr(ws.imp_ws), ws.imp_bytes, _stream()),
        name)


def stage_error_types(dp, ws, slot, tb, per_detection=False):
    """Image-level error breakdown of the pass the workspace holds (after
    stage_ranges .. stage_match): ws.err_dt_counts[n_rng, n_cat, 7],
    ws.err_gt_counts[n_rng, n_cat, 3] and, with `per_detection`,
    ws.err_dt_type[n_dt, n_rng] (taoamd_error_types; the definition is in
    include/tao_amodal_hip.h) at IoU threshold slot `slot` of the calling
    thread's thresholds and background threshold `tb`.  The per-image row lists
    are built once per problem; the match indices come from the existing match
    entry and stay on the device: the workspace's own table (detail mode), else
    error_match_gt(), filled here by one more match with match_gt requested
    unless the caller's match already wrote it.  Buffers are allocated on the
    first call."""
    _error_pass(dp, ws, slot, tb, "lvis", per_detection=per_detection)


def stage_error_impact(dp, ws, slot, tb):
    """The AP each error type costs, of the pass the workspace holds (after
    stage_ranges .. stage_match and the sort): the breakdown once more with its
    links (taoamd_error_types_links: ws.err_link_same, ws.err_link_other
    int32[n_dt, n_rng], ws.err_held uint8[n_rng, n_gt], the types in
    ws.err_dt_type), then the sweep of the nine variants (taoamd_error_impact;
    the definition is in include/tao_amodal_hip.h): ws.imp_precision[9, 101,
    n_cat, n_rng] under the calling thread's recall thresholds and
    ws.imp_num_gt[9, n_cat, n_rng].  Buffers are allocated on the first call and
    kept with the workspace: the two link tables are 8 bytes per (row, range)
    together -- 1.0 GB at 21.4 M rows and 6 ranges --, the sweep's own workspace
    another 4 (`ws.err_link_same = ws.err_link_other = ws.imp_ws = None` gives
    them back)."""
    _error_impact(dp, ws, slot, tb, "lvis")


def stage_track_error_types(dp, ws, slot, tb, per_detection=False):
    """Track-level error breakdown of the pass the workspace holds (after
    stage_ranges .. stage_match): ws.err_dt_counts[n_rng, n_cat, 7],
    ws.err_gt_counts[n_rng, n_cat, 3] and, with `per_detection`,
    ws.err_dt_type[n_dt, n_rng] (taoamd_track_error_types; the definition is in
    include/tao_amodal_hip.h) at IoU threshold slot `slot` of the calling
    thread's thresholds and background threshold `tb`.  The same-category IoUs
    are ws.iou of the pass, the frame-order guard's patches included; the
    cross-category ones are computed here and never stored.  The per-video row
    lists are built once per problem; the match indices come from the
    workspace's own table (detail mode), else from error_match_gt() (800 bytes
    a row), filled here by one more match unless the caller's match already
    wrote it.  Buffers are allocated on the first call."""
    _error_pass(dp, ws, slot, tb, "tao", per_detection=per_detection)


def stage_track_error_impact(dp, ws, slot, tb):
    """The Track-AP each error type costs, of the pass the workspace holds
    (after stage_ranges .. stage_match and the sort): the track-level breakdown
    once more with its links (taoamd_track_error_types_links: ws.err_link_same,
    ws.err_link_other int32[n_dt, n_rng], ws.err_held uint8[n_rng, n_gt], the
    types in ws.err_dt_type), then the sweep of the nine variants
    (taoamd_track_error_impact; the definition is in include/tao_amodal_hip.h):
    ws.imp_precision[9, 101, n_cat, n_rng] under the calling thread's recall
    thresholds and ws.imp_num_gt[9, n_cat, n_rng].  Buffers are allocated on the
    first call and kept with the workspace: the two link tables are 8 bytes per
    (track, range) together -- 58 MB at 361 577 tracks and 20 ranges --, the
    sweep's own workspace another 4 (`ws.err_link_same = ws.err_link_other =
    ws.imp_ws = None` gives them back)."""
    _error_impact(dp, ws, slot, tb, "tao")


def stage_confusion(dp, ws, slot, tb):
    """Which category pairs the CLS and BOTH errors confuse, of the pass the
    workspace holds (after stage_ranges .. stage_match): the level's breakdown
    once more with its links (dp.kind picks taoamd_error_types_links or
    taoamd_track_error_types_links, so the refusals are the breakdown's own),
    then the sparse histogram (taoamd_confusion_count, taoamd_confusion_fill;
    the definition is in include/tao_amodal_hip.h): a CSR over (range, predicted
    category), ws.conf_off int64[n_rng * n_cat + 1], ws.conf_gt_cat int32[n_ent],
    ws.conf_counts int32[n_ent, 4] (cls, both, unheld, adopted); ws.conf_n =
    n_ent.  The number of entries is read between the two calls: one
    synchronisation of the current stream.  Buffers are allocated on the first
    call and kept with the workspace: the link tables as for the impact, 8
    bytes per (row, range) together; the histogram's workspace 12 bytes per
    (range, ground truth) and 4 per (range, category); ws.conf_off 8 bytes per
    (range, category); the entries 20 bytes each, regrown where a call finds
    more (`ws.conf_ws = ws.conf_off = ws.conf_gt_cat = ws.conf_counts = None`
    gives them back)."""
    _error_pass(dp, ws, slot, tb, dp.kind, per_detection=True, links=True)
    lib, t, s = _lib.load(), dp.t, _stream()
    _confusion_buffers(dp, ws, lib)
    tables = (dp.n_dt, dp.n_gt, dp.n_cat, dp.n_rng, _ptr(t["cat_off"]), _ptr(t["dt_score"]),
              _ptr(t["dt_cat"]), _ptr(ws.err_dt_type), _ptr(ws.err_link_other),
              _ptr(t["gt_cat"]), _ptr(ws.err_held), _ptr(ws.conf_off))
    _lib.check(lib.taoamd_confusion_count(*tables, _ptr(ws.conf_ws), ws.conf_bytes, s),
               "taoamd_confusion_count")
    _confusion_entries(dp, ws, int(ws.conf_off[-1].item()))       # (synchronises)
    _lib.check(lib.taoamd_confusion_fill(
        *tables, ws.conf_n, _ptr(ws.conf_gt_cat), _ptr(ws.conf_counts), _ptr(ws.conf_ws),
        ws.conf_bytes, s), "taoamd_confusion_fill")


def set_frame_visibility(dp, vis):
    """The visibility of every ground-truth frame of a track-level problem
    (float64[n_gt_frames], the annotations' `visibility` in the order of
    gt_frame_*): what stage_track_association's windows read.  Uploaded once."""
    vis = np.ascontiguousarray(vis, dtype=np.float64)
    if len(vis) != int(dp.t["gt_frame_pos"].numel()):
        raise _lib.TaoAmdError("%d visibilities for %d ground-truth frames"
                               % (len(vis), int(dp.t["gt_frame_pos"].numel())))
    dp.t["gt_frame_vis"] = torch.from_numpy(vis if len(vis) else np.zeros(1)).to(dp.device)


def _track_tables(dp, what):
    """What the stages of the three track analyses share: the refusal, in the
    stage's own words `what`, and the argument groups of their entry points --
    the sizes (n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames), the cells'
    three offset tables, the six frame tables (detections first)."""
    if dp.kind != "tao" or dp.mask_iou:
        raise _lib.TaoAmdError("the track %s the track level's, on boxes" % what)
    t = dp.t
    sizes = (dp.n_dt, dp.n_gt, dp.n_cells, dp.n_iou,
             int(t["dt_frame_pos"].numel()), int(t["gt_frame_pos"].numel()))
    cells = (_ptr(t["cell_dt_off"]), _ptr(t["cell_gt_off"]), _ptr(t["cell_iou_off"]))
    frames = (_ptr(t["dt_frame_off"]), _ptr(t["dt_frame_pos"]), _ptr(t["dt_frame_box"]),
              _ptr(t["gt_frame_off"]), _ptr(t["gt_frame_pos"]), _ptr(t["gt_frame_box"]))
    return sizes, cells, frames


def _vis_windows(dp, vis_rng):
    """The closed visibility windows of a stage that takes them, as float64[n_vis,
    2], refused where the kernels cannot take them."""
    vis_rng = np.ascontiguousarray(vis_rng if vis_rng is not None else [],
                                   dtype=np.float64).reshape(-1, 2)
    n_vis = len(vis_rng)
    if n_vis > _lib.TRACK_ASSOCIATION_VIS:
        raise _lib.TaoAmdError("%d visibility windows; the kernels take up to %d"
                               % (n_vis, _lib.TRACK_ASSOCIATION_VIS))
    if n_vis and dp.t.get("gt_frame_vis") is None:
        raise _lib.TaoAmdError("visibility windows need the frames' visibility "
                               "(engine.set_frame_visibility)")
    return vis_rng


def _buffer(ws, dev, name, shape, dtype, exact=False):
    """The buffer rule of the on-request stages: ws.<name> is allocated by the first
    call that asks for it and kept with the workspace.  `shape`: an int or a
    tuple.  By default at least shape[0] leading rows of the trailing shape: a
    larger buffer stays, a smaller one is regrown, and the buffer is handed out
    whole -- the kernels take its address; the leading rows are its [:shape[0]]
    (no view is formed here: a slice costs the stages that do not want one
    microseconds between two launches).  exact=True: a buffer of `shape` itself,
    allocated anew where the shape differs, and None (ws.<name> too) for a table
    of no rows: no windows."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    have = getattr(ws, name)
    if have is not None and have.shape == shape:
        return have
    if exact:
        have = torch.empty(shape, dtype=dtype, device=dev) if shape[0] else None
        setattr(ws, name, have)
        return have
    if have is None or have.shape[0] < shape[0] or have.shape[1:] != shape[1:]:
        have = torch.empty(shape, dtype=dtype, device=dev)
        setattr(ws, name, have)
    return have


def _workspace(ws, dev, stage, nbytes):
    """The workspace pair of an on-request stage: ws.<stage>_ws of ws.<stage>_bytes (256
    at least), allocated by the first call and regrown where a call needs more
    than it holds."""
    if getattr(ws, stage + "_ws") is None or getattr(ws, stage + "_bytes") < nbytes:
        setattr(ws, stage + "_bytes", int(nbytes))
        setattr(ws, stage + "_ws",
                torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev))


def _stage_buffers(ws, dev, stage, key, nbytes, buffers):
    """A stage's workspace and buffers under _workspace and _buffer, asked for
    where the stage's last call on this workspace had other sizes `key` (the
    product "<stage> buffers") and only then: nbytes() gives the workspace's
    bytes, buffers() rows of (name, shape, dtype[, exact])."""
    if not _valid(ws, stage + " buffers", key):
        with _producing(ws, stage + " buffers", key):
            _workspace(ws, dev, stage, nbytes())
            for request in buffers():
                _buffer(ws, dev, *request)


def _valid(ws, product, key):
    """Does the workspace hold `product` (a name of ws.valid) for `key`."""
    return ws.valid.get(product) == key


class _producing:
    """The validity rule of what the on-request stages reuse, as a context around the
    lines that write a product: the key is cleared before the first launch that
    writes it and set after the last check passed, so the product is valid for
    no key after the lines raised anywhere.  The products: the results a later
    stage reads ("followers", "share", "identity", at their frame_thr; "match
    indices", the breakdown's, at ()) and each
    stage's own buffers ("<stage> buffers", at the sizes they depend on beyond
    the problem's: a call with the same sizes asks for none again)."""

    def __init__(self, ws, product, key):
        self.valid, self.product, self.key = ws.valid, product, key

    def __enter__(self):
        self.valid.pop(self.product, None)

    def __exit__(self, raised, *_):
        if raised is None:
            self.valid[self.product] = self.key


_SEARCH_BOUND = "a search ran out of its loop bound"


def _raise_on_status(status, name, texts):
    """Reads the status word a stage's kernels left (one synchronisation of the
    current stream); a non-zero code raises in the name of the entry point, with
    texts[code - 1] -- the last text for every greater code."""
    code = int(status.item())
    if code:
        raise _lib.TaoAmdError("%s: status %d (%s)"
                               % (name, code, texts[min(code, len(texts)) - 1]))


def _vis_tables(dp, ws, name, vis_rng, columns):
    """The windows' side of the association and of CLEAR: ws.<name> int64[n_vis,
    n_cat, len(columns)] under the exact rule (None without windows), and the
    arguments (the frames' visibility, the windows' upload, ws.<name>) as
    pointers, None without windows.  Also returns the upload, which the caller
    keeps alive until its kernels ran."""
    n_vis = len(vis_rng)
    rng_t = torch.from_numpy(vis_rng).to(dp.device) if n_vis else None
    counts = _buffer(ws, dp.device, name, (n_vis, dp.n_cat, len(columns)), torch.int64,
                     exact=True)
    return (_ptr(dp.t["gt_frame_vis"]) if n_vis else None, _ptr(rng_t), _ptr(counts)), rng_t


def _identity_share(dp, ws, frame_thr, tables, work):
    """taoamd_track_identity_share at `frame_thr` into ws.ident_share int32[n_iou]
    (the product "share"), in the workspace `work` = (pointer, bytes) of the
    calling stage, which has asked for ws.ident_share: the frame index the call
    builds there is read by its own kernel alone.  `tables` as of _track_tables."""
    sizes, cells, frames = tables
    with _producing(ws, "share", frame_thr):
        _lib.check(_lib.load().taoamd_track_identity_share(
            *sizes, frame_thr, *cells, *frames, _ptr(ws.ident_share), *work, _stream()),
            "taoamd_track_identity_share")


def kept_tracks(dp, ws, frame_thr, keep):
    """The dt_keep table of HOTA and CLEAR: `keep` where the caller brings one,
    else the identity's ws.ident_keep at `frame_thr` -- stage_track_identity
    runs first unless the workspace holds it for that threshold."""
    if keep is not None:
        return keep
    if not _valid(ws, "identity", frame_thr):
        stage_track_identity(dp, ws, frame_thr)
    return ws.ident_keep


def stage_track_association(dp, ws, frame_thr, vis_rng):
    """Per-frame followers of the ground-truth tracks (taoamd_track_association;
    the definition is in include/tao_amodal_hip.h): ws.assoc_follow[n_iou] in the
    layout of the IoU matrix, ws.assoc_gt[n_gt, 7], ws.assoc_cat_counts[n_cat, 8],
    ws.assoc_vis_counts[n_vis, n_cat, 3] (None without windows), ws.assoc_best
    [n_gt_frames] and ws.assoc_best_iou[n_gt_frames], at the per-frame threshold
    `frame_thr` in (0, 1] and the closed visibility windows `vis_rng` (up to 8
    {lo, hi} pairs; they need set_frame_visibility).  On request only.  Reads the
    track tables alone -- never ws.iou, never the match --, so it depends on
    neither the metric, the thresholds nor the ranges.  Buffers are allocated on
    the first call and kept with the workspace.  The followers are the product
    "followers" of ws.valid, at `frame_thr`."""
    lib, t, dev, frame_thr = _lib.load(), dp.t, dp.device, float(frame_thr)
    i32 = torch.int32
    with _producing(ws, "followers", frame_thr):
        sizes, cells, frames = _track_tables(dp, "association is")
        vis_rng = _vis_windows(dp, vis_rng)
        n_gf = sizes[5]
        _stage_buffers(
            ws, dev, "assoc", (),
            lambda: lib.taoamd_track_association_workspace(dp.n_dt, dp.n_gt, n_gf), lambda: (
                ("assoc_follow", max(dp.n_iou, 1), i32),
                ("assoc_gt", (max(dp.n_gt, 1), len(_lib.ASSOC_TRACK_COLUMNS)), i32),
                ("assoc_cat_counts", (dp.n_cat, len(_lib.ASSOC_CAT_COLUMNS)), torch.int64),
                ("assoc_best", max(n_gf, 1), i32),
                ("assoc_best_iou", max(n_gf, 1), torch.float64)))
        # (the windows' upload is read by the kernels of this stream: alive until they ran)
        (vis, rng, vis_counts), ws.assoc_vis_rng = _vis_tables(
            dp, ws, "assoc_vis_counts", vis_rng, _lib.ASSOC_VIS_COLUMNS)
        _lib.check(lib.taoamd_track_association(
            *sizes, dp.n_cat, len(vis_rng), frame_thr, *cells, _ptr(t["gt_cat"]),
            _ptr(t["gt_flags"]), *frames, vis, rng, _ptr(ws.assoc_follow), _ptr(ws.assoc_gt),
            _ptr(ws.assoc_cat_counts), vis_counts, _ptr(ws.assoc_best), _ptr(ws.assoc_best_iou),
            _ptr(ws.assoc_ws), ws.assoc_bytes, _stream()), "taoamd_track_association")


def stage_track_occlusion(dp, ws, frame_thr, vis_lo, vis_hi, recover, len_edges, episodes=False):
    """Is a ground-truth track's follower kept through occlusion
    (taoamd_track_occlusion_count, taoamd_track_occlusion_fill; the definition is
    in include/tao_amodal_hip.h): the runs of frames with vis_lo <= visibility <=
    vis_hi, over the followers ws.assoc_best of stage_track_association at
    `frame_thr` -- reused where the workspace holds them for that threshold, else
    that stage runs first, without windows.  ws.occ_gt int32[n_gt, 4], ws.occ_off
    int64[n_gt + 1] (the tracks' first episode), ws.occ_counts int64[n_cat, n_len,
    11]; with episodes=True also ws.occ_episodes int32[>= n_ep, 9] and ws.occ_n =
    n_ep, read between the two calls: one synchronisation of the current stream
    (ws.occ_n is None otherwise).  `recover` in [1, 64], `len_edges` up to 8
    ascending lengths that start at 1.  Needs set_frame_visibility.  On request
    only.  Buffers are allocated on the first call and kept with the workspace:
    4 bytes per ground-truth track of workspace, 24 per track and 88 per
    (category, bucket) of results, 36 per episode, regrown where a call finds more."""
    sizes, _, frames = _track_tables(dp, "occlusions are")
    n_gf = sizes[5]
    lib, t, dev, s = _lib.load(), dp.t, dp.device, _stream()
    if t.get("gt_frame_vis") is None:
        raise _lib.TaoAmdError("the occlusion episodes need the frames' visibility "
                               "(engine.set_frame_visibility)")
    edges = np.ascontiguousarray(len_edges, dtype=np.int32).reshape(-1)
    n_len = len(edges)
    if not 1 <= n_len <= _lib.TRACK_OCCLUSION_LEN:
        raise _lib.TaoAmdError("%d length buckets; the kernels take 1 to %d"
                               % (n_len, _lib.TRACK_OCCLUSION_LEN))
    frame_thr = float(frame_thr)
    if not _valid(ws, "followers", frame_thr):
        stage_track_association(dp, ws, frame_thr, [])
    _stage_buffers(
        ws, dev, "occ", n_len,
        lambda: lib.taoamd_track_occlusion_workspace(dp.n_gt, n_gf, n_len), lambda: (
            ("occ_gt", (max(dp.n_gt, 1), len(_lib.OCC_TRACK_COLUMNS)), torch.int32),
            ("occ_off", dp.n_gt + 1, torch.int64),
            ("occ_counts", (dp.n_cat, n_len, len(_lib.OCC_COUNT_COLUMNS)), torch.int64, True)))
    work = (_ptr(ws.occ_ws), ws.occ_bytes, s)
    tables = (dp.n_gt, n_gf, dp.n_cat, n_len, int(recover), float(vis_lo), float(vis_hi),
              edges.ctypes.data, _ptr(t["gt_cat"]), _ptr(t["gt_flags"]),
              frames[3], _ptr(t["gt_frame_vis"]), _ptr(ws.assoc_best))
    _lib.check(lib.taoamd_track_occlusion_count(
        *tables, _ptr(ws.occ_gt), _ptr(ws.occ_off), _ptr(ws.occ_counts), *work),
        "taoamd_track_occlusion_count")
    ws.occ_n = None
    if not episodes:
        return
    ws.occ_n = int(ws.occ_off[-1].item())           # (synchronises)
    ep = _buffer(ws, dev, "occ_episodes", (max(ws.occ_n, 1), len(_lib.OCC_EPISODE_COLUMNS)),
                 torch.int32)
    _lib.check(lib.taoamd_track_occlusion_fill(
        *tables, _ptr(ws.occ_off), ws.occ_n, _ptr(ep), *work), "taoamd_track_occlusion_fill")


def stage_track_identity(dp, ws, frame_thr):
    """IDF1 / IDP / IDR from an optimal one-to-one assignment of detection tracks
    to ground-truth tracks per cell (taoamd_track_identity_share,
    taoamd_track_identity_assign; the definition is in include/tao_amodal_hip.h):
    ws.ident_share int32[n_iou] in the layout of the IoU matrix -- per pair the
    frames with a box IoU >= `frame_thr` in (0, 1] --, ws.ident_cat_counts
    int64[n_cat, 6], ws.ident_gt int32[n_gt, 2] = {the assigned detection row or
    -1, its share}, ws.ident_dt int32[n_dt, 2] = {the assigned ground-truth row or
    -1, kept}, ws.ident_keep uint8[n_dt] = that `kept` column as the dt_keep table
    HOTA and CLEAR read.  The four tables of the assignment are the product
    "identity" of ws.valid at `frame_thr`; ws.ident_share is a product of its
    own ("share"), written by every call of this stage and by
    stage_track_identity_at where it needs another threshold's.  On request
    only.  Reads the track tables alone, like
    stage_track_association.  Raises if the assignment kernel reports a non-zero
    status (an exhausted loop bound, weights beyond 64-bit potentials): one
    synchronisation of the current stream.  Buffers are allocated
    on the first call and kept with the workspace: 4 bytes per pair of a cell, 8
    per track and 1 more per detection track, and a workspace of 56 bytes per
    detection track, 44 per ground-truth track and 4 per ground-truth frame."""
    lib, t, dev, frame_thr = _lib.load(), dp.t, dp.device, float(frame_thr)
    i32 = torch.int32
    with _producing(ws, "identity", frame_thr):
        sizes, cells, frames = tables = _track_tables(dp, "identity is")
        _stage_buffers(
            ws, dev, "ident", (),
            lambda: lib.taoamd_track_identity_workspace(dp.n_dt, dp.n_gt, sizes[5]), lambda: (
                ("ident_share", max(dp.n_iou, 1), i32),
                ("ident_cat_counts", (dp.n_cat, len(_lib.IDENT_CAT_COLUMNS)), torch.int64),
                ("ident_gt", (max(dp.n_gt, 1), 2), i32), ("ident_dt", (max(dp.n_dt, 1), 2), i32),
                ("ident_keep", max(dp.n_dt, 1), torch.uint8), ("ident_status", 1, i32)))
        work = (_ptr(ws.ident_ws), ws.ident_bytes)
        _identity_share(dp, ws, frame_thr, tables, work)
        _lib.check(lib.taoamd_track_identity_assign(
            *sizes, dp.n_cat, *cells, _ptr(t["gt_cat"]), _ptr(t["gt_flags"]), _ptr(t["dt_cat"]),
            _ptr(t["dt_flags"]), frames[0], frames[3], _ptr(ws.ident_share),
            _ptr(ws.ident_cat_counts), _ptr(ws.ident_gt), _ptr(ws.ident_dt),
            _ptr(ws.ident_status), *work, _stream()), "taoamd_track_identity_assign")
        ws.ident_keep.copy_(ws.ident_dt[:, 1])
        _raise_on_status(ws.ident_status, "taoamd_track_identity_assign",
                         (_SEARCH_BOUND, "a cell's weights exceed 64-bit potentials"))


def _thr_table(dp, thr_table):
    """A table of track-level score thresholds as float64[n_thr, n_cat], refused
    where the kernels cannot take it."""
    thr = np.ascontiguousarray(thr_table, dtype=np.float64)
    if thr.ndim != 2 or thr.shape[1] != dp.n_cat:
        raise _lib.TaoAmdError("a threshold table of shape %s; [n_thr, %d] is the tables'"
                               % (thr.shape, dp.n_cat))
    if not 1 <= len(thr) <= _lib.TRACK_SCORE_THRS:
        raise _lib.TaoAmdError("%d threshold layers; the kernels take 1 to %d"
                               % (len(thr), _lib.TRACK_SCORE_THRS))
    return thr


def stage_track_score_pass(dp, ws, thr_table, base):
    """Which detection tracks lie at or above a score (taoamd_track_score_pass;
    the rule is in include/tao_amodal_hip.h, section "track-level score
    thresholds"): ws.at_pass uint8[n_thr, n_dt], 1 where dt_score >= `thr_table`
    [layer, the track's category] (float64[n_thr, n_cat], 1 to 64 layers) and
    `base` -- a uint8[n_dt] device tensor or None -- is not 0 there.  Returns it.
    On request only; a buffer of its own, regrown where a call brings more layers."""
    _track_tables(dp, "score thresholds are")
    lib, t, dev = _lib.load(), dp.t, dp.device
    thr = _thr_table(dp, thr_table)
    n_thr = len(thr)
    if t["dt_score"].dtype != torch.float64:
        raise _lib.TaoAmdError("dt_score is %s; the pass rule reads doubles" % t["dt_score"].dtype)
    out = _buffer(ws, dev, "at_pass", (n_thr, max(dp.n_dt, 1)), torch.uint8)[:n_thr]
    thr_t = torch.from_numpy(thr).to(dev)
    _lib.check(lib.taoamd_track_score_pass(
        dp.n_dt, dp.n_cat, n_thr, _ptr(t["dt_score"]), _ptr(t["dt_cat"]), _ptr(thr_t), _ptr(base),
        _ptr(out), _stream()), "taoamd_track_score_pass")
    ws.at_thr = thr_t      # (read by the kernel of this stream: alive until it ran)
    return out


def stage_track_identity_at(dp, ws, frame_thr, thr_table, per_track=False):
    """The identity's assignment over the detection tracks at or above a score,
    a layer per row of `thr_table` float64[n_thr, n_cat] in ONE launch
    (taoamd_track_score_pass, taoamd_track_identity_assign_at; the definition is
    in include/tao_amodal_hip.h, section "track-level score thresholds"):
    ws.at_cat_counts int64[n_thr, n_cat, 6], ws.at_dt int32[n_thr, n_dt, 2],
    ws.at_keep uint8[n_thr, n_dt] = the layers' kept columns (kept AND pass: what
    stage_track_hota and stage_track_clear take as `keep`), and with
    per_track=True ws.at_gt int32[n_thr, n_gt, 2] (None otherwise).  share runs
    once for all layers, and not at all where ws.ident_share holds the shares at
    `frame_thr` (the product "share": of stage_track_identity or of an earlier
    call of this stage); it is the one buffer the two stages have in common,
    and nothing else stage_track_identity left is written.  Raises on a
    non-zero status: one synchronisation of the current stream.  The workspace
    is the identity's with 44 bytes per track and layer, regrown where a call
    brings more layers."""
    sizes, cells, frames = tables = _track_tables(dp, "identity is")
    lib, t, dev, s = _lib.load(), dp.t, dp.device, _stream()
    thr = _thr_table(dp, thr_table)
    n_thr, frame_thr = len(thr), float(frame_thr)
    _stage_buffers(
        ws, dev, "at", n_thr,
        lambda: lib.taoamd_track_identity_layers_workspace(dp.n_dt, dp.n_gt, sizes[5], n_thr),
        lambda: (("at_status", 1, torch.int32), ("ident_share", max(dp.n_iou, 1), torch.int32)))
    work = (_ptr(ws.at_ws), ws.at_bytes)
    if not _valid(ws, "share", frame_thr):
        _identity_share(dp, ws, frame_thr, tables, work)
    passed = stage_track_score_pass(dp, ws, thr, None)
    ws.at_cat_counts = torch.empty((n_thr, dp.n_cat, len(_lib.IDENT_CAT_COLUMNS)),
                                   dtype=torch.int64, device=dev)
    ws.at_dt = torch.empty((n_thr, max(dp.n_dt, 1), 2), dtype=torch.int32, device=dev)
    ws.at_gt = torch.empty((n_thr, max(dp.n_gt, 1), 2), dtype=torch.int32, device=dev) \
        if per_track else None
    _lib.check(lib.taoamd_track_identity_assign_at(
        *sizes, dp.n_cat, n_thr, *cells, _ptr(t["gt_cat"]), _ptr(t["gt_flags"]),
        _ptr(t["dt_cat"]), _ptr(t["dt_flags"]), _ptr(passed), frames[0], frames[3],
        _ptr(ws.ident_share), _ptr(ws.at_cat_counts), _ptr(ws.at_gt), _ptr(ws.at_dt),
        _ptr(ws.at_status), *work, s), "taoamd_track_identity_assign_at")
    ws.at_keep = ws.at_dt[:, :, 1].to(torch.uint8).contiguous()
    _raise_on_status(ws.at_status, "taoamd_track_identity_assign_at",
                     (_SEARCH_BOUND, "a cell's weights exceed 64-bit potentials"))


def stage_track_hota(dp, ws, alphas, frame_thr, keep=None):
    """HOTA's integer tables from a one-to-one assignment per frame
    (taoamd_track_hota_align, taoamd_track_hota_match, taoamd_track_hota_reduce;
    the definition is in include/tao_amodal_hip.h): ws.hota_tp and ws.hota_loc
    int64[n_cat, n_alpha], ws.hota_ass int64[n_cat, n_alpha, 3] in fixed point
    (_lib.HOTA_ONE), ws.hota_match int32[n_gt_frames] (the in-cell index of the
    frame's detection track or -1) and ws.hota_match_iou, at the ascending
    localisation thresholds `alphas` (1 to 32 doubles, TrackEval's eps already
    subtracted).  The detection tracks that take part are the identity's kept
    ones at `frame_thr`: stage_track_identity runs first unless the workspace
    holds it for that threshold (the product "identity" of ws.valid) -- or, with
    `keep`, the tracks of that uint8[n_dt] device tensor (a layer of ws.at_keep
    of stage_track_identity_at), and the identity is neither run nor read.  On
    request only.  Raises
    if the match reports a non-zero status (an exhausted loop bound): one
    synchronisation of the current stream.  Buffers are allocated on the first
    call and kept with the workspace: 8 bytes per pair of a cell for pot and 12
    per (alpha, pair) for mc and lc, regrown where a call brings more alphas, 12
    per ground-truth frame, and a workspace of 64 bytes
    per detection track, 68 per ground-truth track and 4 per ground-truth frame."""
    sizes, cells, frames = _track_tables(dp, "HOTA is")
    lib, t, dev, s = _lib.load(), dp.t, dp.device, _stream()
    alphas = np.ascontiguousarray(alphas, dtype=np.float64).reshape(-1)
    n_alpha = len(alphas)
    if not 1 <= n_alpha <= _lib.TRACK_HOTA_ALPHAS:
        raise _lib.TaoAmdError("%d alphas; the kernels take 1 to %d"
                               % (n_alpha, _lib.TRACK_HOTA_ALPHAS))
    keep = kept_tracks(dp, ws, float(frame_thr), keep)
    n_gf, n_iou, i32, i64 = max(sizes[5], 1), max(dp.n_iou, 1), torch.int32, torch.int64
    _stage_buffers(
        ws, dev, "hota", n_alpha,
        lambda: lib.taoamd_track_hota_workspace(dp.n_dt, dp.n_gt, sizes[5]), lambda: (
            ("hota_pot", n_iou, i64), ("hota_mc", (n_alpha, n_iou), i32),
            ("hota_lc", (n_alpha, n_iou), i64), ("hota_match", n_gf, i32),
            ("hota_match_iou", n_gf, torch.float64), ("hota_status", 1, i32)))
    ws.hota_tp = torch.empty((dp.n_cat, n_alpha), dtype=torch.int64, device=dev)
    ws.hota_loc = torch.empty((dp.n_cat, n_alpha), dtype=torch.int64, device=dev)
    ws.hota_ass = torch.empty((dp.n_cat, n_alpha, 3), dtype=torch.int64, device=dev)
    tables = (*cells, _ptr(t["gt_flags"]), _ptr(keep), *frames)
    work = (_ptr(ws.hota_ws), ws.hota_bytes, s)
    _lib.check(lib.taoamd_track_hota_align(*sizes, *tables, _ptr(ws.hota_pot), *work),
               "taoamd_track_hota_align")
    _lib.check(lib.taoamd_track_hota_match(
        *sizes, n_alpha, alphas.ctypes.data, *tables, _ptr(ws.hota_pot), _ptr(ws.hota_mc),
        _ptr(ws.hota_lc), _ptr(ws.hota_match), _ptr(ws.hota_match_iou), _ptr(ws.hota_status),
        *work), "taoamd_track_hota_match")
    _lib.check(lib.taoamd_track_hota_reduce(
        *sizes, dp.n_cat, n_alpha, *cells, _ptr(t["gt_cat"]), _ptr(t["gt_flags"]), frames[0],
        frames[3], _ptr(ws.hota_mc), _ptr(ws.hota_lc), _ptr(ws.hota_tp), _ptr(ws.hota_loc),
        _ptr(ws.hota_ass), *work), "taoamd_track_hota_reduce")
    _raise_on_status(ws.hota_status, "taoamd_track_hota_match", (_SEARCH_BOUND,))


def stage_track_clear(dp, ws, frame_thr, vis_rng, keep=None):
    """CLEAR MOT's integer tables from a one-to-one assignment per step that
    depends on the step before (taoamd_track_clear_count, _fill, _walk, _reduce;
    the definition is in include/tao_amodal_hip.h): ws.clear_cat_counts
    int64[n_cat, 7] (motp_sum in fixed point, _lib.HOTA_ONE), ws.clear_vis_counts
    int64[n_vis, n_cat, 4] (None without windows), ws.clear_gt int32[n_gt, 4],
    ws.clear_match int32[n_gt_frames] (the in-cell index of the frame's detection
    track or -1), ws.clear_match_iou and ws.clear_sw uint8[n_gt_frames], at the
    per-frame threshold `frame_thr` in (0, 1] and the closed visibility windows
    `vis_rng` (up to 8 {lo, hi} pairs; they need set_frame_visibility).  The
    detection tracks that take part are the identity's kept ones at `frame_thr`:
    stage_track_identity runs first unless the workspace holds it for that
    threshold (the product "identity" of ws.valid) -- or, with `keep`, the tracks
    of that uint8[n_dt] device tensor, as for stage_track_hota.  On request
    only.  The number of candidates is
    read between count and fill, the status word at the end: two synchronisations
    of the current stream; a non-zero status raises.  Buffers are allocated on the
    first call and kept with the workspace: 22 bytes per ground-truth frame, 16
    per candidate (regrown where a call finds more), 16 per ground-truth track,
    and a workspace of 144 bytes per detection track, 132 per
    ground-truth track and 8 per ground-truth frame."""
    sizes, cells, frames = _track_tables(dp, "CLEAR is")
    lib, t, dev, s = _lib.load(), dp.t, dp.device, _stream()
    vis_rng = _vis_windows(dp, vis_rng)
    frame_thr = float(frame_thr)
    keep = kept_tracks(dp, ws, frame_thr, keep)
    n_dt, n_gt, n_cells, _, n_df, n_gf = sizes
    i32, f64, u8 = torch.int32, torch.float64, torch.uint8
    _stage_buffers(
        ws, dev, "clear", (), lambda: lib.taoamd_track_clear_workspace(n_dt, n_gt, n_gf), lambda: (
            ("clear_off", n_gf + 1, torch.int64), ("clear_step", max(n_gf, 1), u8),
            ("clear_match", max(n_gf, 1), i32), ("clear_match_iou", max(n_gf, 1), f64),
            ("clear_sw", max(n_gf, 1), u8), ("clear_status", 1, i32),
            ("clear_gt", (max(n_gt, 1), len(_lib.CLEAR_TRACK_COLUMNS)), i32),
            ("clear_cat_counts", (dp.n_cat, len(_lib.CLEAR_CAT_COLUMNS)), torch.int64)))
    work = (_ptr(ws.clear_ws), ws.clear_bytes, s)
    off, step, match, sw, gt = (_ptr(ws.clear_off), _ptr(ws.clear_step), _ptr(ws.clear_match),
                                _ptr(ws.clear_sw), _ptr(ws.clear_gt))
    tables = (n_dt, n_gt, n_cells, n_df, n_gf, frame_thr, cells[0], cells[1],
              _ptr(t["gt_flags"]), _ptr(keep), *frames)
    _lib.check(lib.taoamd_track_clear_count(*tables, off, step, *work),
               "taoamd_track_clear_count")
    ws.clear_n = int(ws.clear_off[-1].item())       # (synchronises)
    ws.clear_cand = tuple(_buffer(ws, dev, name, max(ws.clear_n, 1), dtype) for name, dtype in
                          (("clear_row", i32), ("clear_q", i32), ("clear_iou", f64)))
    row, q, iou = map(_ptr, ws.clear_cand)
    _lib.check(lib.taoamd_track_clear_fill(*tables, off, ws.clear_n, row, q, iou, *work),
               "taoamd_track_clear_fill")
    _lib.check(lib.taoamd_track_clear_walk(
        n_dt, n_gt, n_cells, n_gf, ws.clear_n, cells[0], cells[1], _ptr(t["gt_flags"]),
        frames[3], frames[4], off, row, q, iou, step, match, _ptr(ws.clear_match_iou), sw, gt,
        _ptr(ws.clear_status), *work), "taoamd_track_clear_walk")
    (vis, rng, vis_counts), rng_t = _vis_tables(dp, ws, "clear_vis_counts", vis_rng,
                                                _lib.CLEAR_VIS_COLUMNS)
    _lib.check(lib.taoamd_track_clear_reduce(
        n_dt, n_gt, n_gf, ws.clear_n, dp.n_cat, len(vis_rng), _ptr(t["gt_cat"]),
        _ptr(t["gt_flags"]), frames[3], vis, rng, off, row, q, match, sw, gt,
        _ptr(ws.clear_cat_counts), vis_counts, *work), "taoamd_track_clear_reduce")
    # (synchronises: the windows' upload rng_t was read while this frame held it)
    _raise_on_status(ws.clear_status, "taoamd_track_clear_walk", (
        _SEARCH_BOUND, "a cell's smaller side exceeds %d" % _lib.TRACK_CLEAR_NMAX))


def stage_track_iou_guarded(dp, ws):
    stage_track_iou(dp, ws)
    stage_iou_guard(dp, ws)
    if dp.guard_flat is not None:
        # host half of the guard (ids Python does not hash to themselves):
        # one synchronisation, the listed pairs patched before the match
        ws.guarded_pairs = apply_iou_guard(dp, ws)


STAGES = (("ranges", stage_ranges), ("sort", stage_sort),
          ("track_iou", stage_track_iou_guarded), ("match", stage_match),
          ("accumulate", stage_accumulate))


def run(dp, ws):
    """Launch one evaluator pass on the current stream (asynchronous, unless
    the problem needs the host half of the frame-order guard)."""
    if _lib.TIMING:
        _lib.kernel_timing_label(dp.kind)
    for name, fn in STAGES:
        fn(dp, ws)


class Overlap:
    """Runs evaluator passes concurrently on separate HIP streams.

    Every kernel of this path is latency / dependency bound (rocprofv3 SQ
    counters: 20-45 % active cycles), so independent work fills the idle
    issue slots: the image-level and the track-level pass share nothing, and
    inside a pass range masks, sort and 3D IoU only meet at the match kernel.
    Streams are forked from / joined to the caller's current stream with
    events, so the caller's barrier + synchronize bracketing stays valid."""

    def __init__(self, device, n=4):
        self.device = torch.device(device)
        self.streams = [torch.cuda.Stream(self.device) for _ in range(n)]

    def _fork(self, k):
        s = self.streams[k]
        s.wait_stream(torch.cuda.current_stream(self.device))
        return s

    def run_pair(self, dpl, wsl, dpt, wst):
        # The image-level chain is the longer one (sort -> match -> six sweep
        # kernels): it stays on the caller's stream, so nothing on it waits
        # for a cross-stream event at the step's start or end (measured:
        # 0.479 -> 0.464 ms against forking both passes); only the track-level
        # pass is forked and joined.
        cur = torch.cuda.current_stream(self.device)
        s_aux_l, s_aux_t = self.streams[2], self.streams[3]   # forked by run_forked
        st = self._fork(1)
        run_forked(dpl, wsl, s_aux_l)
        with torch.cuda.stream(st):
            run_forked(dpt, wst, s_aux_t)
        cur.wait_stream(st)


class StageProbe:
    """HIP events around single-kernel stages, recorded on the stream the
    kernel is launched on while the (overlapped) steps run: the dominant
    kernels' launch durations inside the timed region of bench.py."""

    def __init__(self):
        self.events = {}

    def wrap(self, name, fn, dp, ws):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn(dp, ws)
        b.record()
        self.events.setdefault(name, []).append((a, b))

    def mean_ms(self):
        """(call after a synchronize)"""
        return {k: sum(a.elapsed_time(b) for a, b in v) / len(v)
                for k, v in self.events.items()}


PROBE = None     # set to a StageProbe to time stage_track_iou / stage_match


def _probed(name, fn, dp, ws):
    if PROBE is None:
        fn(dp, ws)
    else:
        PROBE.wrap(dp.kind + ":" + name, fn, dp, ws)


def run_forked(dp, ws, aux, head_only=False, sort_aside=None):
    """One evaluator pass on the current stream, its independent head stages
    on the stream `aux` (forked from and joined to the current stream):
    image level  ranges || sort -> match -> accumulate,
    track level  (ranges, sort) || 3D IoU -> match -> accumulate.
    `sort_aside` (image level; None: where the workspace was built for it,
    Workspace.gather): the match leaves its rows in cell order -- it reads no
    dst[], stores full wavefront runs and the sort stores order[] alone -- and
    the sweep gathers them through order[]."""
    cur = torch.cuda.current_stream(dp.device)
    aux.wait_stream(cur)
    if _lib.TIMING:
        _lib.kernel_timing_label(dp.kind)
    if sort_aside is None:
        sort_aside = ws.gather and _plan_key(dp)[1] in (2, 3)
    if sort_aside and dp.kind == "lvis" and not dp.mask_iou and not head_only \
            and dp.grouped and dp.n_dt:
        order_only = sort_is_sampled(dp) and ws.order_buf is not None
        if order_only and not ws.dst_identity:
            # nobody stores sorted places: dst[] says where the rows are
            torch.arange(dp.n_dt, out=ws.dst[:dp.n_dt])
            ws.dst_identity = True
        # the match BESIDE the sort (it no longer depends on it), not behind it:
        # 1.290-1.304 against 1.327-1.335 ms a step at 21 M rows (parent 1.356-1.361)
        with torch.cuda.stream(aux):
            stage_sort(dp, ws, order_only=order_only)
        stage_ranges(dp, ws)
        _probed("match", lambda d, w: stage_match(d, w, scatter=False), dp, ws)
        cur.wait_stream(aux)
        stage_accumulate_by_order(dp, ws)
        return
    if dp.kind == "lvis":
        with torch.cuda.stream(aux):
            stage_ranges(dp, ws)
            stage_mask_iou(dp, ws)
        stage_sort(dp, ws)
    else:
        with torch.cuda.stream(aux):
            stage_ranges(dp, ws)
            stage_sort(dp, ws)
        _probed("track_iou", stage_track_iou_guarded, dp, ws)
    cur.wait_stream(aux)
    _probed("match", stage_match, dp, ws)
    if not head_only:
        stage_accumulate(dp, ws)


def time_stages(dpl, wsl, dpt, wst, reps=10):
    """Average duration (ms) of every stage of both evaluators, measured with
    HIP events recorded on the stream the kernels are launched on."""
    out = {}
    for side, dp, ws in (("lvis", dpl, wsl), ("tao", dpt, wst)):
        acc = {name: 0.0 for name, _ in STAGES}
        for _ in range(reps):
            evs = []
            for name, fn in STAGES:
                a = torch.cuda.Event(enable_timing=True)
                b = torch.cuda.Event(enable_timing=True)
                a.record()
                fn(dp, ws)
                b.record()
                evs.append((name, a, b))
            torch.cuda.synchronize(dp.device)
            for name, a, b in evs:
                acc[name] += a.elapsed_time(b)
        out[side] = {k: round(v / reps, 4) for k, v in acc.items()}
    return out


def run_guarded(dp, ws, flat=None, upto=None, read_count=True, head=True, match_gt=None):
    """One evaluator pass; returns the number of pairs the frame-order guard
    recomputed (synchronises at the end to read it, unless read_count=False:
    guarded_pairs() gives it later).  `head=False`: a further pass over the
    SAME detections under other evaluation constants (blocks of thresholds /
    ranges, evaluation/_core.py) -- the score order and the IoU matrix of the
    pass before it stand (neither depends on a threshold or a range); the
    range masks, the guard's near list (it is taken against the thresholds;
    pairs it patched earlier keep the reference-order value) and the match
    are what is repeated."""
    if _lib.TIMING:
        _lib.kernel_timing_label(dp.kind)
    stage_ranges(dp, ws)
    if head:
        stage_sort(dp, ws)
        stage_track_iou(dp, ws)
    stage_iou_guard(dp, ws)
    apply_iou_guard(dp, ws, flat)
    if match_gt is None:
        stage_match(dp, ws)
    else:
        stage_match(dp, ws, match_gt=match_gt)
    if upto != "match":
        stage_accumulate(dp, ws)
    if not read_count:
        return None
    ws.guarded_pairs = guarded_pairs(dp, ws)
    return ws.guarded_pairs


def evaluate_flat(flat, device="cuda", detail=False, iou_3d_type="3d_iou",
                  guard="device"):
    """Upload, run, download.  Returns a dict of numpy arrays shaped like the
    C oracle's outputs (tests compare the two field by field)."""
    dp = DeviceProblem(flat, device, iou_3d_type, guard=guard)
    ws = Workspace(dp, detail=detail, dt_rng_table=True)
    guarded = run_guarded(dp, ws, flat)
    torch.cuda.synchronize(dp.device)
    n = dp.n_dt
    out = {
        "precision": ws.precision.cpu().numpy(),
        "recall": ws.recall.cpu().numpy(),
        "num_gt": ws.num_gt.cpu().numpy(),
        "gt_rng": ws.gt_rng[:dp.n_gt].cpu().numpy().view(np.uint32),
        "dt_rng": ws.dt_rng[:n].cpu().numpy().view(np.uint32),
        "order": ws.order[:n].cpu().numpy().astype(np.int64),
        "dst": ws.dst[:n].cpu().numpy().astype(np.int64),
        # rows are in sorted order on the device; give them back per detection
        "matched_sorted": ws.matched[:n].cpu().numpy().view(np.uint64),
        "ignored_sorted": ws.ignored[:n].cpu().numpy().view(np.uint64),
    }
    out["matched"] = out["matched_sorted"][out["dst"]] if n else out["matched_sorted"]
    out["ignored"] = out["ignored_sorted"][out["dst"]] if n else out["ignored_sorted"]
    if dp.kind == "tao":
        out["iou"] = ws.iou[:dp.n_iou].cpu().numpy()
        out["pairs"] = int(ws.pair_frames.item())
        out["near_threshold_pairs"] = guarded
    if detail:
        out["match_gt"] = ws.match_gt[:n].cpu().numpy()
        if dp.kind == "lvis" and not dp.mask_iou:
            out["iou"] = ws.ious_out[:dp.n_iou].cpu().numpy()
    if dp.mask_iou:
        out["iou"] = ws.iou[:dp.n_iou].cpu().numpy()
    return out
