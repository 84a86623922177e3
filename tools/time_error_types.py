#!/usr/bin/env python
"""Measurement of the error breakdowns (taoamd_error_types,
taoamd_track_error_types) on the synthetic configurations of bench.py, with HIP
events:

    python tools/time_error_types.py [--level image|track] [--config 3s] [--reps 20] [--warmup 3]
                                     [--impact] [--association] [--occlusions] [--identity]
                                     [--hota] [--clear] [--curve [N]] [--confusion]

Times, on the image level's tables of that configuration, each alone on an idle
stream: the fused match as a benchmark step runs it (the yardstick), the
detail-mode match that produces match_gt (existing code the breakdown depends
on), and the breakdown itself with and without the per-detection table; lists
the breakdown's kernels and the pair counts that bound it (an image's
detections x ALL its ground truths against the match's same-category pairs).
--level track times, on the track table of the configuration: stage_track_iou of
a benchmark step (the same-category pairs), the plan-less taoamd_track_iou on
the cells pooled per video (every pair of a video, the cross-category ones done
naively), the match that produces match_gt, and the breakdown; lists its kernels
and the (pair, shared frame) counts.  --impact adds the error impact: the
breakdown with its links (taoamd_error_types_links; --level track:
taoamd_track_error_types_links), the links pass followed by the sweep of the
nine variants (engine.stage_error_impact / engine.stage_track_error_impact),
the kernels of both, and AP and dAP over all categories in range 0.  --level
track --association times, instead of the breakdown, the per-frame followers
(engine.stage_track_association) and the plan-less taoamd_track_iou over the
same cells in the same process.  --level track --occlusions times the occlusion
episodes (engine.stage_track_occlusion: count and fill each alone, the whole
stage) beside the association pass they follow, in the same process.  --level
track --identity times the identity measures: taoamd_track_identity_share and
taoamd_track_identity_assign each alone between HIP events and the whole stage
(engine.stage_track_identity), beside the association pass without windows in
the same process.  --level track --hota times HOTA: taoamd_track_hota_align,
taoamd_track_hota_match and taoamd_track_hota_reduce each alone between HIP
events and the whole stage (engine.stage_track_hota) beside the identity stage
in the same process, and reports the sizes of mc and lc and the share of frame
groups with more than one ground truth.  --level track --clear times CLEAR MOT:
the candidates (taoamd_track_clear_count and _fill), taoamd_track_clear_walk and
taoamd_track_clear_reduce each alone between HIP events and the whole stage
(engine.stage_track_clear) beside the identity and the HOTA stage in the same
process, and reports the number of candidates, the share of steps with more than
one ground truth and the sizes of the candidate store and the workspace.
--level track --curve [N] times the track-level score thresholds at N (default
10) thresholds, the default ones of tracking_curve(): taoamd_track_score_pass
alone, taoamd_track_identity_assign_at over the N layers in ONE launch against
the same layers as N launches of one layer each, the thresholded identity stage
(engine.stage_track_identity_at) and the whole curve (that stage, then HOTA and
CLEAR once per layer) beside the unthresholded identity, HOTA and CLEAR stages in
the same process; reports the kept tracks, IDF1, HOTA and MOTA per threshold.
--confusion
(both levels) adds the confusion table: the level's links pass,
taoamd_confusion_count and taoamd_confusion_fill, each alone between HIP events
in the same process, the whole stage with its read of the entry count, the
kernels, and the number of entries beside the cells of the dense table.  Prints
one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CONFIGS = {"2": (200, 300, 50), "3s": (2000, 300, 50), "5s": (10000, 1, 1000)}


def timed_calls(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"min_ms": round(min(out), 4), "median_ms": round(float(np.median(out)), 4),
            "max_ms": round(max(out), 4)}


def pooled_cells(dp, lists):
    """The track table's frame lists regrouped so that a video is ONE cell: what
    the plan-less taoamd_track_iou needs to compute every (detection track,
    ground-truth track) pair of a video.  On the device."""
    import torch
    _, vid_gt_off, vid_gt, vid_dt_off, vid_dt = lists
    t = dp.t
    out = {}
    for side, rows, n in (("dt", vid_dt, dp.n_dt), ("gt", vid_gt, dp.n_gt)):
        rows = rows[:n].long()
        off = t[side + "_frame_off"].long()
        cnt = (off[1:] - off[:-1])[rows]
        new_off = torch.zeros(n + 1, dtype=torch.int64, device=rows.device)
        new_off[1:] = torch.cumsum(cnt, 0)
        take = torch.repeat_interleave(off[rows] - new_off[:-1], cnt) \
            + torch.arange(int(new_off[-1]), device=rows.device)
        out[side + "_frame_off"] = new_off.to(torch.int32)
        out[side + "_frame_pos"] = t[side + "_frame_pos"][take].contiguous()
        out[side + "_frame_box"] = t[side + "_frame_box"][take].contiguous()
    d_cnt = (vid_dt_off[1:] - vid_dt_off[:-1]).long()
    g_cnt = (vid_gt_off[1:] - vid_gt_off[:-1]).long()
    iou_off = torch.zeros(len(d_cnt) + 1, dtype=torch.int64, device=d_cnt.device)
    iou_off[1:] = torch.cumsum(d_cnt * g_cnt, 0)
    out.update(cell_dt_off=vid_dt_off, cell_gt_off=vid_gt_off, cell_iou_off=iou_off,
               n_cells=len(d_cnt), n_pairs=int(iou_off[-1]))
    return out


def track_level(a, gt, dt, dev, V):
    import torch
    from tao_amodal_amd import _lib, engine, flatten, flatten_dev
    dt.track_id, _ = flatten.make_track_ids_unique(dt)
    fl = flatten_dev.flatten_tao(gt, dt, device=dev)
    dp = engine.DeviceProblem(fl, dev)
    ws = engine.Workspace(dp)
    engine.run_guarded(dp, ws, fl, upto="match", read_count=False)
    torch.cuda.synchronize()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        return timed_calls(fn, a.warmup, a.reps)
    res = {"level": "track", "config": a.config, "videos": V, "rows": dp.n_dt,
           "ground_truths": dp.n_gt, "categories": dp.n_cat, "cells": dp.n_cells,
           "same_category_pairs": dp.n_iou,
           "same_category_pair_frames": int(ws.pair_frames.item()),
           "dt_frames": int(dp.t["dt_frame_pos"].numel()),
           "gt_frames": int(dp.t["gt_frame_pos"].numel())}
    res["track_iou_step"] = timed(lambda: engine.stage_track_iou(dp, ws))
    if a.association:
        return association(a, res, gt, fl, dp, ws, timed)
    if a.occlusions:
        return occlusions(a, res, gt, fl, dp, ws, timed)
    if a.identity:
        return identity(a, res, dp, ws, timed)
    if a.hota:
        return hota(a, res, dp, ws, timed)
    if a.clear:
        return clear(a, res, gt, fl, dp, ws, timed)
    if a.curve:
        return curve(a, res, fl, dp, ws, timed)
    res["match_fused"] = timed(lambda: engine.stage_match(dp, ws))
    # the first call builds the per-video lists and runs the match for match_gt
    engine.stage_track_error_types(dp, ws, 0, a.bg_thr)
    torch.cuda.synchronize()
    res["match_with_match_gt"] = timed(
        lambda: engine.stage_match(dp, ws, match_gt=ws.err_match_gt))
    res["track_error_types"] = timed(
        lambda: engine.stage_track_error_types(dp, ws, 0, a.bg_thr))
    res["track_error_types_per_detection"] = timed(
        lambda: engine.stage_track_error_types(dp, ws, 0, a.bg_thr, per_detection=True))
    _lib.kernel_timing(True)
    for _ in range(a.reps):
        engine.stage_track_error_types(dp, ws, 0, a.bg_thr)
    res["kernels_ms"] = {k: round(ms / n, 4) for k, (ms, n) in _lib.kernel_timings().items()}
    _lib.kernel_timing(False)
    res["dt_counts_by_type_range0"] = ws.err_dt_counts[0].sum(0).tolist()
    res["gt_counts_range0"] = ws.err_gt_counts[0].sum(0).tolist()
    # the second yardstick: every pair of a video through the plan-less kernel
    p = pooled_cells(dp, dp.err_tabs)
    res["video_pairs"] = p["n_pairs"]
    res["cross_category_pairs"] = p["n_pairs"] - dp.n_iou
    iou = torch.empty(max(p["n_pairs"], 1), dtype=torch.float64, device=dev)
    frames = torch.zeros(1, dtype=torch.int64, device=dev)

    def naive():
        _lib.check(lib.taoamd_track_iou(
            p["n_cells"], p["cell_dt_off"].data_ptr(), p["cell_gt_off"].data_ptr(),
            p["cell_iou_off"].data_ptr(), p["n_pairs"], p["dt_frame_off"].data_ptr(),
            p["dt_frame_pos"].data_ptr(), p["dt_frame_box"].data_ptr(),
            p["gt_frame_off"].data_ptr(), p["gt_frame_pos"].data_ptr(),
            p["gt_frame_box"].data_ptr(), 0, iou.data_ptr(), frames.data_ptr(), stream),
            "taoamd_track_iou")
    res["track_iou_planless_video_pooled"] = timed(naive)
    res["video_pair_frames"] = int(frames.item())
    res["cross_category_pair_frames"] = res["video_pair_frames"] - res["same_category_pair_frames"]
    if a.impact:
        # the first call allocates the link tables and the sweep's workspace
        engine.stage_track_error_impact(dp, ws, 0, a.bg_thr)
        torch.cuda.synchronize()
        res["track_error_types_links"] = timed(
            lambda: engine._error_pass(dp, ws, 0, a.bg_thr, dp.kind, per_detection=True,
                                       links=True))
        res["track_error_impact_links_and_sweep"] = timed(
            lambda: engine.stage_track_error_impact(dp, ws, 0, a.bg_thr))
        _lib.kernel_timing(True)
        for _ in range(a.reps):
            engine.stage_track_error_impact(dp, ws, 0, a.bg_thr)
        res["impact_kernels_ms"] = {k: round(ms / n, 4)
                                    for k, (ms, n) in _lib.kernel_timings().items()}
        _lib.kernel_timing(False)
        res["impact_sweep_kernels_ms"] = round(sum(
            v for k, v in res["impact_kernels_ms"].items() if k.startswith("imp_")), 4)
        res["impact_workspace_bytes"] = int(ws.imp_bytes)
        res["link_table_bytes"] = int(ws.err_link_same.numel() + ws.err_link_other.numel()) * 4
        p = ws.imp_precision[..., 0].cpu().numpy()
        ap_ = [float(v[v > -1].mean()) if (v > -1).any() else -1.0 for v in p]
        res["fixes"] = list(_lib.ERROR_FIXES)
        res["ap_range0"] = [round(v, 6) for v in ap_]
        res["dap_range0"] = [round(v - ap_[0], 6) for v in ap_[1:]]
    if a.confusion:
        confusion(a, res, dp, ws, timed)
    print(json.dumps(res))


def confusion(a, res, dp, ws, timed):
    """--confusion: the links pass of the level, then taoamd_confusion_count and
    taoamd_confusion_fill on its tables, each alone; engine.stage_confusion as a
    whole (links, count, the read of the entry count, fill)."""
    import torch
    from tao_amodal_amd import _lib, engine
    lib = _lib.load()
    # the first call allocates the link tables, the workspace and the entries
    engine.stage_confusion(dp, ws, 0, a.bg_thr)
    torch.cuda.synchronize()
    t, stream = dp.t, torch.cuda.current_stream().cuda_stream
    tables = (dp.n_dt, dp.n_gt, dp.n_cat, dp.n_rng, t["cat_off"].data_ptr(),
              t["dt_score"].data_ptr(), t["dt_cat"].data_ptr(), ws.err_dt_type.data_ptr(),
              ws.err_link_other.data_ptr(), t["gt_cat"].data_ptr(), ws.err_held.data_ptr(),
              ws.conf_off.data_ptr())

    def count():
        _lib.check(lib.taoamd_confusion_count(*tables, ws.conf_ws.data_ptr(), ws.conf_bytes,
                                              stream), "taoamd_confusion_count")

    def fill():
        _lib.check(lib.taoamd_confusion_fill(
            *tables, ws.conf_n, ws.conf_gt_cat.data_ptr(), ws.conf_counts.data_ptr(),
            ws.conf_ws.data_ptr(), ws.conf_bytes, stream), "taoamd_confusion_fill")
    res["confusion_links_pass"] = timed(
        lambda: engine._error_pass(dp, ws, 0, a.bg_thr, dp.kind, per_detection=True,
                                   links=True))
    res["confusion_count"] = timed(count)
    res["confusion_fill"] = timed(fill)
    res["confusion_stage"] = timed(lambda: engine.stage_confusion(dp, ws, 0, a.bg_thr))
    _lib.kernel_timing(True)
    for _ in range(a.reps):
        count()
        fill()
    res["confusion_kernels_ms"] = {k: round(ms / n, 4)
                                   for k, (ms, n) in _lib.kernel_timings().items()}
    _lib.kernel_timing(False)
    res["confusion_entries"] = int(ws.conf_n)
    res["confusion_dense_cells"] = dp.n_rng * dp.n_cat * dp.n_cat
    res["confusion_workspace_bytes"] = int(ws.conf_bytes)
    res["confusion_entry_bytes"] = 20 * int(ws.conf_n) + 8 * int(ws.conf_off.numel())
    off0 = int(ws.conf_off[dp.n_cat].item())
    res["confusion_columns"] = list(_lib.CONFUSION_COLUMNS)
    res["confusion_counts_range0"] = ws.conf_counts[:off0].sum(0).tolist() if off0 else [0] * 4


def association(a, res, gt, fl, dp, ws, timed):
    """--level track --association: the per-frame followers
    (engine.stage_track_association) at frame_thr 0.5 with the five default
    visibility windows and without windows, its kernels, and -- in the same
    process -- the plan-less taoamd_track_iou over the SAME cells: the same
    (detection track, ground-truth track) pairs and the same shared frames."""
    import torch
    from tao_amodal_amd import _lib, engine
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    windows = [[0, 1.0], [0, 0.1], [0.1, 0.8], [0.8, 1.0], [0, 0.8]]
    engine.set_frame_visibility(dp, np.asarray(gt.ann_vis)[fl.gt_frame_box.index])
    # the first call allocates the buffers
    engine.stage_track_association(dp, ws, 0.5, windows)
    torch.cuda.synchronize()
    res["track_association"] = timed(lambda: engine.stage_track_association(dp, ws, 0.5, windows))
    res["track_association_no_windows"] = timed(
        lambda: engine.stage_track_association(dp, ws, 0.5, []))
    _lib.kernel_timing(True)
    for _ in range(a.reps):
        engine.stage_track_association(dp, ws, 0.5, windows)
    res["kernels_ms"] = {k: round(ms / n, 4) for k, (ms, n) in _lib.kernel_timings().items()}
    _lib.kernel_timing(False)
    res["association_workspace_bytes"] = int(ws.assoc_bytes)
    tot = ws.assoc_cat_counts.sum(0).tolist()
    res["cat_counts_total"] = dict(zip(_lib.ASSOC_CAT_COLUMNS, tot))
    res["vis_counts_total"] = ws.assoc_vis_counts.sum(1).tolist()
    t = dp.t
    iou = torch.empty(max(dp.n_iou, 1), dtype=torch.float64, device=dp.device)
    frames = torch.zeros(1, dtype=torch.int64, device=dp.device)

    def naive():
        _lib.check(lib.taoamd_track_iou(
            dp.n_cells, t["cell_dt_off"].data_ptr(), t["cell_gt_off"].data_ptr(),
            t["cell_iou_off"].data_ptr(), dp.n_iou, t["dt_frame_off"].data_ptr(),
            t["dt_frame_pos"].data_ptr(), t["dt_frame_box"].data_ptr(),
            t["gt_frame_off"].data_ptr(), t["gt_frame_pos"].data_ptr(),
            t["gt_frame_box"].data_ptr(), 0, iou.data_ptr(), frames.data_ptr(), stream),
            "taoamd_track_iou")
    res["track_iou_planless_same_cells"] = timed(naive)
    res["planless_pair_frames"] = int(frames.item())
    _lib.kernel_timing(True)
    for _ in range(a.reps):
        naive()
    res["planless_kernels_ms"] = {k: round(ms / n, 4)
                                  for k, (ms, n) in _lib.kernel_timings().items()}
    _lib.kernel_timing(False)
    print(json.dumps(res))


def occlusions(a, res, gt, fl, dp, ws, timed):
    """--level track --occlusions: the occlusion episodes
    (engine.stage_track_occlusion) at frame_thr 0.5, window [0, 0.1], recover 3
    and the default length buckets, in the same process as the association pass
    whose followers they read: that pass without windows, taoamd_track_occlusion_count
    and taoamd_track_occlusion_fill each alone between HIP events, the whole stage
    without and with the records (the latter reads the episode count), and the
    kernels of both passes."""
    import torch
    from tao_amodal_amd import _lib, engine
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    thr, lo, hi, recover, edges = 0.5, 0.0, 0.1, 3, (1, 3, 6, 11)
    engine.set_frame_visibility(dp, np.asarray(gt.ann_vis)[fl.gt_frame_box.index])
    # the first call allocates the buffers of both passes and the records
    engine.stage_track_occlusion(dp, ws, thr, lo, hi, recover, edges, episodes=True)
    torch.cuda.synchronize()
    res["track_association_no_windows"] = timed(
        lambda: engine.stage_track_association(dp, ws, thr, []))
    t, n_gf = dp.t, int(dp.t["gt_frame_pos"].numel())
    e = np.ascontiguousarray(edges, dtype=np.int32)
    tables = (dp.n_gt, n_gf, dp.n_cat, len(e), recover, lo, hi, e.ctypes.data,
              t["gt_cat"].data_ptr(), t["gt_flags"].data_ptr(), t["gt_frame_off"].data_ptr(),
              t["gt_frame_vis"].data_ptr(), ws.assoc_best.data_ptr())

    def count():
        _lib.check(lib.taoamd_track_occlusion_count(
            *tables, ws.occ_gt.data_ptr(), ws.occ_off.data_ptr(), ws.occ_counts.data_ptr(),
            ws.occ_ws.data_ptr(), ws.occ_bytes, stream), "taoamd_track_occlusion_count")

    def fill():
        _lib.check(lib.taoamd_track_occlusion_fill(
            *tables, ws.occ_off.data_ptr(), n_ep, ws.occ_episodes.data_ptr(),
            ws.occ_ws.data_ptr(), ws.occ_bytes, stream), "taoamd_track_occlusion_fill")
    n_ep = int(ws.occ_n)
    res["occlusion_count"] = timed(count)
    res["occlusion_fill"] = timed(fill)
    res["occlusion_stage"] = timed(
        lambda: engine.stage_track_occlusion(dp, ws, thr, lo, hi, recover, edges))
    res["occlusion_stage_with_episodes"] = timed(
        lambda: engine.stage_track_occlusion(dp, ws, thr, lo, hi, recover, edges, episodes=True))
    _lib.kernel_timing(True)
    for _ in range(a.reps):
        engine.stage_track_association(dp, ws, thr, [])
        count()
        fill()
    res["kernels_ms"] = {k: round(ms / n, 4) for k, (ms, n) in _lib.kernel_timings().items()}
    _lib.kernel_timing(False)
    res["occlusion_episodes"] = n_ep
    res["occlusion_workspace_bytes"] = int(ws.occ_bytes)
    res["occlusion_bytes_read"] = 12 * n_gf
    res["occlusion_columns"] = list(_lib.OCC_COUNT_COLUMNS)
    res["occlusion_counts_by_bucket"] = ws.occ_counts.sum(0).tolist()
    print(json.dumps(res))


def identity(a, res, dp, ws, timed):
    """--level track --identity: the identity measures (engine.stage_track_identity)
    at frame_thr 0.5: taoamd_track_identity_share and taoamd_track_identity_assign
    each alone between HIP events, the whole stage (which reads the status word),
    the association pass without windows in the same process, the kernels of the
    three, and what the assignment met: the cells with a pair to assign, the
    largest sides, the totals."""
    import torch
    from tao_amodal_amd import _lib, engine
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    thr = 0.5
    # the first calls allocate the buffers of both passes
    engine.stage_track_identity(dp, ws, thr)
    engine.stage_track_association(dp, ws, thr, [])
    torch.cuda.synchronize()
    t = dp.t
    sizes = (dp.n_dt, dp.n_gt, dp.n_cells, dp.n_iou, int(t["dt_frame_pos"].numel()),
             int(t["gt_frame_pos"].numel()))
    cells = (t["cell_dt_off"].data_ptr(), t["cell_gt_off"].data_ptr(),
             t["cell_iou_off"].data_ptr())

    def share():
        _lib.check(lib.taoamd_track_identity_share(
            *sizes, thr, *cells, t["dt_frame_off"].data_ptr(), t["dt_frame_pos"].data_ptr(),
            t["dt_frame_box"].data_ptr(), t["gt_frame_off"].data_ptr(),
            t["gt_frame_pos"].data_ptr(), t["gt_frame_box"].data_ptr(),
            ws.ident_share.data_ptr(), ws.ident_ws.data_ptr(), ws.ident_bytes, stream),
            "taoamd_track_identity_share")

    def assign():
        _lib.check(lib.taoamd_track_identity_assign(
            *sizes, dp.n_cat, *cells, t["gt_cat"].data_ptr(), t["gt_flags"].data_ptr(),
            t["dt_cat"].data_ptr(), t["dt_flags"].data_ptr(), t["dt_frame_off"].data_ptr(),
            t["gt_frame_off"].data_ptr(), ws.ident_share.data_ptr(),
            ws.ident_cat_counts.data_ptr(), ws.ident_gt.data_ptr(), ws.ident_dt.data_ptr(),
            ws.ident_status.data_ptr(), ws.ident_ws.data_ptr(), ws.ident_bytes, stream),
            "taoamd_track_identity_assign")
    res["track_association_no_windows"] = timed(
        lambda: engine.stage_track_association(dp, ws, thr, []))
    res["identity_share"] = timed(share)
    res["identity_assign"] = timed(assign)
    res["identity_stage"] = timed(lambda: engine.stage_track_identity(dp, ws, thr))
    _lib.kernel_timing(True)
    for _ in range(a.reps):
        engine.stage_track_association(dp, ws, thr, [])
        share()
        assign()
    res["kernels_ms"] = {k: round(ms / n, 4) for k, (ms, n) in _lib.kernel_timings().items()}
    _lib.kernel_timing(False)
    torch.cuda.synchronize()
    # what the assignment met, from the share matrix (on the device, untimed)
    sh = ws.ident_share[:dp.n_iou]
    cell_of = torch.repeat_interleave(
        torch.arange(dp.n_cells, device=sh.device),
        (t["cell_iou_off"][1:] - t["cell_iou_off"][:-1]).long())
    hit = torch.zeros(dp.n_cells, dtype=torch.int64, device=sh.device)
    hit.index_add_(0, cell_of, (sh > 0).long())
    res["identity_status"] = int(ws.ident_status.item())
    res["identity_pairs_with_share"] = int((sh > 0).sum().item())
    res["identity_cells_with_share"] = int((hit > 0).sum().item())
    res["identity_most_pairs_with_share_in_a_cell"] = int(hit.max().item()) if dp.n_cells else 0
    res["identity_share_max"] = int(sh.max().item()) if dp.n_iou else 0
    res["identity_largest_cell"] = [
        int((t["cell_dt_off"][1:] - t["cell_dt_off"][:-1]).max().item()),
        int((t["cell_gt_off"][1:] - t["cell_gt_off"][:-1]).max().item())]
    res["identity_workspace_bytes"] = int(ws.ident_bytes)
    res["identity_share_bytes"] = 4 * dp.n_iou
    res["identity_columns"] = list(_lib.IDENT_CAT_COLUMNS)
    tot = ws.ident_cat_counts.sum(0).tolist()
    res["identity_totals"] = tot
    res["idf1"] = round(2 * tot[4] / max(tot[1] + tot[3], 1), 6)
    print(json.dumps(res))


def hota(a, res, dp, ws, timed):
    """--level track --hota: HOTA (engine.stage_track_hota) at TrackEval's 19
    alphas over the identity's kept tracks at frame_thr 0.5: the three calls each
    alone between HIP events, the whole stage (which reads the status word), the
    identity stage in the same process, the kernels, the sizes of the tables and
    the share of frame groups with more than one ground truth."""
    import torch
    from tao_amodal_amd import _lib, engine
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    thr = 0.5
    alphas = np.ascontiguousarray(np.arange(0.05, 0.99, 0.05) - np.finfo(float).eps)
    n_alpha = len(alphas)
    # the first call allocates the buffers of both stages
    engine.stage_track_hota(dp, ws, alphas, thr)
    torch.cuda.synchronize()
    t = dp.t
    sizes = (dp.n_dt, dp.n_gt, dp.n_cells, dp.n_iou, int(t["dt_frame_pos"].numel()),
             int(t["gt_frame_pos"].numel()))
    cells = (t["cell_dt_off"].data_ptr(), t["cell_gt_off"].data_ptr(),
             t["cell_iou_off"].data_ptr())
    tables = (*cells, t["gt_flags"].data_ptr(), ws.ident_keep.data_ptr(),
              t["dt_frame_off"].data_ptr(), t["dt_frame_pos"].data_ptr(),
              t["dt_frame_box"].data_ptr(), t["gt_frame_off"].data_ptr(),
              t["gt_frame_pos"].data_ptr(), t["gt_frame_box"].data_ptr())

    def align():
        _lib.check(lib.taoamd_track_hota_align(
            *sizes, *tables, ws.hota_pot.data_ptr(), ws.hota_ws.data_ptr(), ws.hota_bytes,
            stream), "taoamd_track_hota_align")

    def match():
        _lib.check(lib.taoamd_track_hota_match(
            *sizes, n_alpha, alphas.ctypes.data, *tables, ws.hota_pot.data_ptr(),
            ws.hota_mc.data_ptr(), ws.hota_lc.data_ptr(), ws.hota_match.data_ptr(),
            ws.hota_match_iou.data_ptr(), ws.hota_status.data_ptr(), ws.hota_ws.data_ptr(),
            ws.hota_bytes, stream), "taoamd_track_hota_match")

    def reduce():
        _lib.check(lib.taoamd_track_hota_reduce(
            *sizes, dp.n_cat, n_alpha, *cells, t["gt_cat"].data_ptr(), t["gt_flags"].data_ptr(),
            t["dt_frame_off"].data_ptr(), t["gt_frame_off"].data_ptr(), ws.hota_mc.data_ptr(),
            ws.hota_lc.data_ptr(), ws.hota_tp.data_ptr(), ws.hota_loc.data_ptr(),
            ws.hota_ass.data_ptr(), ws.hota_ws.data_ptr(), ws.hota_bytes, stream),
            "taoamd_track_hota_reduce")
    res["identity_stage"] = timed(lambda: engine.stage_track_identity(dp, ws, thr))
    res["hota_align"] = timed(align)
    res["hota_match"] = timed(match)
    res["hota_reduce"] = timed(reduce)
    res["hota_stage"] = timed(lambda: engine.stage_track_hota(dp, ws, alphas, thr))
    _lib.kernel_timing(True)
    for _ in range(a.reps):
        align()
        match()
        reduce()
    res["kernels_ms"] = {k: round(ms / n, 4) for k, (ms, n) in _lib.kernel_timings().items()}
    _lib.kernel_timing(False)
    torch.cuda.synchronize()
    # what the match met (on the device, untimed): a frame group is (cell, position);
    # its ground truths are the eligible ones with a frame there
    n_gf = sizes[5]
    foff = t["gt_frame_off"].long()
    g_of = torch.repeat_interleave(torch.arange(dp.n_gt, device=foff.device), foff[1:] - foff[:-1])
    g_cell = torch.repeat_interleave(
        torch.arange(dp.n_cells, device=foff.device),
        (t["cell_gt_off"][1:] - t["cell_gt_off"][:-1]).long())
    elig = (t["gt_flags"][:dp.n_gt][g_of] & 1) == 0
    top = int(t["gt_frame_pos"].max().item()) + 1 if n_gf else 1
    key = g_cell[g_of].long() * top + t["gt_frame_pos"].long()
    _, per_group = torch.unique(key[elig], return_counts=True)
    res["hota_status"] = int(ws.hota_status.item())
    res["hota_alphas"] = n_alpha
    res["hota_frame_groups"] = int(per_group.numel())
    res["hota_frame_groups_with_several_ground_truths"] = int((per_group > 1).sum().item())
    res["hota_largest_frame_group"] = int(per_group.max().item()) if per_group.numel() else 0
    res["hota_matched_frames"] = int((ws.hota_match[:n_gf] >= 0).sum().item())
    res["hota_workspace_bytes"] = int(ws.hota_bytes)
    res["hota_pot_bytes"] = 8 * dp.n_iou
    res["hota_mc_bytes"] = 4 * n_alpha * dp.n_iou
    res["hota_lc_bytes"] = 8 * n_alpha * dp.n_iou
    tp = ws.hota_tp.sum(0).double()
    ass = ws.hota_ass.sum(0).double()[:, 0] / _lib.HOTA_ONE
    cc = ws.ident_cat_counts.sum(0).tolist()
    deta = tp / torch.clamp(cc[1] + cc[3] - tp, min=1)
    assa = ass / torch.clamp(tp, min=1)
    res["hota_totals"] = {"gt_frames": cc[1], "dt_frames": cc[3], "tp": [int(x) for x in tp.tolist()]}
    res["hota"] = round(float(torch.sqrt(deta * assa).mean().item()), 6)
    print(json.dumps(res))


def clear(a, res, gt, fl, dp, ws, timed):
    """--level track --clear: CLEAR MOT (engine.stage_track_clear) over the
    identity's kept tracks at frame_thr 0.5 with the association's five windows:
    the candidates (count and fill), the walk and the reduction each alone between
    HIP events, the whole stage (which reads the candidate count and the status
    word), the identity and the HOTA stage in the same process, the kernels, the
    number of candidates, the share of steps with more than one ground truth and
    the sizes of the candidate store and the workspace."""
    import torch
    from tao_amodal_amd import _lib, engine
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    thr = 0.5
    windows = np.array([[0, 1.0], [0, 0.1], [0.1, 0.8], [0.8, 1.0], [0, 0.8]])
    alphas = np.ascontiguousarray(np.arange(0.05, 0.99, 0.05) - np.finfo(float).eps)
    engine.set_frame_visibility(dp, np.asarray(gt.ann_vis)[fl.gt_frame_box.index])
    # the first calls allocate the buffers of the three stages
    engine.stage_track_hota(dp, ws, alphas, thr)
    engine.stage_track_clear(dp, ws, thr, windows)
    torch.cuda.synchronize()
    t = dp.t
    n_df, n_gf = int(t["dt_frame_pos"].numel()), int(t["gt_frame_pos"].numel())
    n_cand = int(ws.clear_n)
    row, q, iou = ws.clear_cand
    rng_t = torch.from_numpy(windows).to(dp.device)
    tables = (dp.n_dt, dp.n_gt, dp.n_cells, n_df, n_gf, thr, t["cell_dt_off"].data_ptr(),
              t["cell_gt_off"].data_ptr(), t["gt_flags"].data_ptr(), ws.ident_keep.data_ptr(),
              t["dt_frame_off"].data_ptr(), t["dt_frame_pos"].data_ptr(),
              t["dt_frame_box"].data_ptr(), t["gt_frame_off"].data_ptr(),
              t["gt_frame_pos"].data_ptr(), t["gt_frame_box"].data_ptr())
    store = (ws.clear_off.data_ptr(), row.data_ptr(), q.data_ptr())
    work = (ws.clear_ws.data_ptr(), ws.clear_bytes, stream)

    def count():
        _lib.check(lib.taoamd_track_clear_count(
            *tables, ws.clear_off.data_ptr(), ws.clear_step.data_ptr(), *work),
            "taoamd_track_clear_count")

    def fill():
        _lib.check(lib.taoamd_track_clear_fill(
            *tables, ws.clear_off.data_ptr(), n_cand, row.data_ptr(), q.data_ptr(),
            iou.data_ptr(), *work), "taoamd_track_clear_fill")

    def walk():
        _lib.check(lib.taoamd_track_clear_walk(
            dp.n_dt, dp.n_gt, dp.n_cells, n_gf, n_cand, t["cell_dt_off"].data_ptr(),
            t["cell_gt_off"].data_ptr(), t["gt_flags"].data_ptr(), t["gt_frame_off"].data_ptr(),
            t["gt_frame_pos"].data_ptr(), *store, iou.data_ptr(), ws.clear_step.data_ptr(),
            ws.clear_match.data_ptr(), ws.clear_match_iou.data_ptr(), ws.clear_sw.data_ptr(),
            ws.clear_gt.data_ptr(), ws.clear_status.data_ptr(), *work), "taoamd_track_clear_walk")

    def reduce():
        _lib.check(lib.taoamd_track_clear_reduce(
            dp.n_dt, dp.n_gt, n_gf, n_cand, dp.n_cat, len(windows), t["gt_cat"].data_ptr(),
            t["gt_flags"].data_ptr(), t["gt_frame_off"].data_ptr(), t["gt_frame_vis"].data_ptr(),
            rng_t.data_ptr(), *store, ws.clear_match.data_ptr(), ws.clear_sw.data_ptr(),
            ws.clear_gt.data_ptr(), ws.clear_cat_counts.data_ptr(),
            ws.clear_vis_counts.data_ptr(), *work), "taoamd_track_clear_reduce")
    res["identity_stage"] = timed(lambda: engine.stage_track_identity(dp, ws, thr))
    res["hota_stage"] = timed(lambda: engine.stage_track_hota(dp, ws, alphas, thr))
    res["clear_count"] = timed(count)
    res["clear_fill"] = timed(fill)
    res["clear_walk"] = timed(walk)
    res["clear_reduce"] = timed(reduce)
    res["clear_stage"] = timed(lambda: engine.stage_track_clear(dp, ws, thr, windows))
    _lib.kernel_timing(True)
    for _ in range(a.reps):
        engine.stage_track_hota(dp, ws, alphas, thr)
        count()
        fill()
        walk()
        reduce()
    res["kernels_ms"] = {k: round(ms / n, 4) for k, (ms, n) in _lib.kernel_timings().items()}
    _lib.kernel_timing(False)
    torch.cuda.synchronize()
    # what the walk met (on the device, untimed): a step is a (cell, position) with
    # the step bit; its ground truths are the eligible ones with a frame there
    foff = t["gt_frame_off"].long()
    g_of = torch.repeat_interleave(torch.arange(dp.n_gt, device=foff.device), foff[1:] - foff[:-1])
    g_cnt = (t["cell_gt_off"][1:] - t["cell_gt_off"][:-1]).long()
    g_cell = torch.repeat_interleave(torch.arange(dp.n_cells, device=foff.device), g_cnt)
    on = ws.clear_step[:n_gf] != 0
    top = int(t["gt_frame_pos"].max().item()) + 1 if n_gf else 1
    key = g_cell[g_of].long() * top + t["gt_frame_pos"].long()
    _, per_step = torch.unique(key[on], return_counts=True)
    elig = (t["gt_flags"][:dp.n_gt] & 1) == 0
    per_cell = torch.zeros(dp.n_cells, dtype=torch.int64, device=foff.device)
    per_cell.index_add_(0, g_cell, elig.long())
    n_per = (ws.clear_off[1:] - ws.clear_off[:-1])
    res["clear_status"] = int(ws.clear_status.item())
    res["clear_candidates"] = n_cand
    res["clear_most_candidates_of_a_frame"] = int(n_per.max().item()) if n_gf else 0
    res["clear_steps"] = int(per_step.numel())
    res["clear_steps_with_several_ground_truths"] = int((per_step > 1).sum().item())
    res["clear_cells_with_one_eligible_ground_truth"] = int((per_cell == 1).sum().item())
    res["clear_cells_with_several"] = int((per_cell > 1).sum().item())
    res["clear_store_bytes"] = 8 * (n_gf + 1) + n_gf + 16 * n_cand
    res["clear_workspace_bytes"] = int(ws.clear_bytes)
    cc = ws.ident_cat_counts.sum(0).tolist()
    tot = ws.clear_cat_counts.sum(0).tolist()
    res["clear_columns"] = list(_lib.CLEAR_CAT_COLUMNS)
    res["clear_totals"] = {"gt_frames": cc[1], "dt_frames": cc[3], "counts": tot,
                           "vis_counts": ws.clear_vis_counts.sum(1).tolist()}
    res["mota"] = round((tot[0] - (cc[3] - tot[0]) - tot[1]) / max(cc[1], 1), 6)
    res["motp"] = round(tot[6] / _lib.HOTA_ONE / max(tot[0], 1), 6)
    print(json.dumps(res))


def curve(a, res, fl, dp, ws, timed):
    """--level track --curve N: the track-level score thresholds at frame_thr 0.5
    and N thresholds (the quantiles tracking_curve() takes by default, each applied
    to every category): the pass kernel alone, the layered assignment in one
    launch and as N launches of one layer, the thresholded identity stage, and the
    whole curve -- that stage, then engine.stage_track_hota and stage_track_clear
    per layer, as GpuRun.curve_tables runs them -- beside the unthresholded
    stages in the same process."""
    import torch
    from tao_amodal_amd import _lib, engine
    from tao_amodal_amd.evaluation.tao_amodal.followers import default_score_thrs
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    thr = 0.5
    alphas = np.ascontiguousarray(np.arange(0.05, 0.99, 0.05) - np.finfo(float).eps)
    score = np.asarray(fl.dt_score, dtype=np.float64)
    fin = score[np.isfinite(score)]
    thrs = default_score_thrs(score) if a.curve == 10 else \
        np.unique(np.quantile(fin, np.arange(a.curve) / float(a.curve), method="lower"))
    T = len(thrs)
    table = np.ascontiguousarray(np.repeat(thrs[:, None], dp.n_cat, axis=1))
    # the first calls allocate the buffers of every stage
    engine.stage_track_hota(dp, ws, alphas, thr)
    engine.stage_track_clear(dp, ws, thr, [])
    engine.stage_track_identity_at(dp, ws, thr, table)
    torch.cuda.synchronize()
    t = dp.t
    sizes = (dp.n_dt, dp.n_gt, dp.n_cells, dp.n_iou, int(t["dt_frame_pos"].numel()),
             int(t["gt_frame_pos"].numel()))
    cells = (t["cell_dt_off"].data_ptr(), t["cell_gt_off"].data_ptr(),
             t["cell_iou_off"].data_ptr())
    table_t = torch.from_numpy(table).to(dp.device)
    passed = torch.empty((T, max(dp.n_dt, 1)), dtype=torch.uint8, device=dp.device)
    cat_counts = torch.empty((T, dp.n_cat, 6), dtype=torch.int64, device=dp.device)
    dt_ident = torch.empty((T, max(dp.n_dt, 1), 2), dtype=torch.int32, device=dp.device)
    status = torch.empty(1, dtype=torch.int32, device=dp.device)

    def score_pass():
        _lib.check(lib.taoamd_track_score_pass(
            dp.n_dt, dp.n_cat, T, t["dt_score"].data_ptr(), t["dt_cat"].data_ptr(),
            table_t.data_ptr(), None, passed.data_ptr(), stream), "taoamd_track_score_pass")

    def assign_at(first, n):
        _lib.check(lib.taoamd_track_identity_assign_at(
            *sizes, dp.n_cat, n, *cells, t["gt_cat"].data_ptr(), t["gt_flags"].data_ptr(),
            t["dt_cat"].data_ptr(), t["dt_flags"].data_ptr(), passed[first].data_ptr(),
            t["dt_frame_off"].data_ptr(), t["gt_frame_off"].data_ptr(),
            ws.ident_share.data_ptr(), cat_counts[first].data_ptr(), None,
            dt_ident[first].data_ptr(), status.data_ptr(), ws.at_ws.data_ptr(), ws.at_bytes,
            stream), "taoamd_track_identity_assign_at")

    def looped():
        for k in range(T):
            assign_at(k, 1)

    def whole():
        engine.stage_track_identity_at(dp, ws, thr, table)
        for k in range(T):
            engine.stage_track_hota(dp, ws, alphas, thr, keep=ws.at_keep[k])
            engine.stage_track_clear(dp, ws, thr, [], keep=ws.at_keep[k])
    score_pass()
    res["curve_thresholds"] = [float(x) for x in thrs]
    res["identity_stage"] = timed(lambda: engine.stage_track_identity(dp, ws, thr))
    res["hota_stage"] = timed(lambda: engine.stage_track_hota(dp, ws, alphas, thr))
    res["clear_stage_no_windows"] = timed(lambda: engine.stage_track_clear(dp, ws, thr, []))
    res["score_pass"] = timed(score_pass)
    res["assign_at_one_launch"] = timed(lambda: assign_at(0, T))
    one = cat_counts.clone()
    res["assign_at_one_layer_per_launch"] = timed(looped)
    res["assign_at_launches_agree"] = bool(torch.equal(one, cat_counts))
    res["assign_one_layer"] = timed(lambda: assign_at(0, 1))
    res["identity_at_stage"] = timed(
        lambda: engine.stage_track_identity_at(dp, ws, thr, table))
    res["curve_whole"] = timed_calls(whole, 1, max(a.reps // 4, 3))
    _lib.kernel_timing(True)
    for _ in range(a.reps):
        score_pass()
        assign_at(0, T)
    res["kernels_ms"] = {k: round(ms / n, 4) for k, (ms, n) in _lib.kernel_timings().items()}
    _lib.kernel_timing(False)
    torch.cuda.synchronize()
    res["curve_status"] = int(status.item())
    res["curve_workspace_bytes"] = int(ws.at_bytes)
    res["identity_workspace_bytes"] = int(ws.ident_bytes)
    # what the curve says (untimed): the totals per threshold
    rows = []
    whole()
    cc = ws.at_cat_counts.sum(1).tolist()
    for k in range(T):
        engine.stage_track_hota(dp, ws, alphas, thr, keep=ws.at_keep[k])
        engine.stage_track_clear(dp, ws, thr, [], keep=ws.at_keep[k])
        tp = ws.hota_tp.sum(0).double()
        ass = ws.hota_ass.sum(0).double()[:, 0] / _lib.HOTA_ONE
        deta = tp / torch.clamp(cc[k][1] + cc[k][3] - tp, min=1)
        assa = ass / torch.clamp(tp, min=1)
        tot = ws.clear_cat_counts.sum(0).tolist()
        rows.append({"dt_tracks": cc[k][2],
                     "idf1": round(2 * cc[k][4] / max(cc[k][1] + cc[k][3], 1), 6),
                     "hota": round(float(torch.sqrt(deta * assa).mean().item()), 6),
                     "mota": round((tot[0] - (cc[k][3] - tot[0]) - tot[1]) / max(cc[k][1], 1), 6),
                     "idsw": tot[1]})
    res["curve_rows"] = rows
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", choices=("image", "track"), default="image")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="3s")
    ap.add_argument("--videos", type=int, default=None)
    ap.add_argument("--cats", type=int, default=1203)
    ap.add_argument("--seed", type=int, default=20240807)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bg-thr", type=float, default=0.1)
    ap.add_argument("--impact", action="store_true")
    ap.add_argument("--association", action="store_true")
    ap.add_argument("--occlusions", action="store_true")
    ap.add_argument("--identity", action="store_true")
    ap.add_argument("--hota", action="store_true")
    ap.add_argument("--clear", action="store_true")
    ap.add_argument("--curve", type=int, nargs="?", const=10, default=0,
                    help="thresholds of the tracking curve (1 to 64; 10 when given bare)")
    ap.add_argument("--confusion", action="store_true")
    a = ap.parse_args()
    if a.curve and a.level != "track":
        ap.error("--curve is the track level's: --level track")
    if not 0 <= a.curve <= 64:
        ap.error("--curve takes 1 to 64 thresholds")
    if a.association and a.level != "track":
        ap.error("--association is the track level's: --level track")
    if a.occlusions and a.level != "track":
        ap.error("--occlusions is the track level's: --level track")
    if a.identity and a.level != "track":
        ap.error("--identity is the track level's: --level track")
    if a.hota and a.level != "track":
        ap.error("--hota is the track level's: --level track")
    if a.clear and a.level != "track":
        ap.error("--clear is the track level's: --level track")
    import torch
    from tao_amodal_amd import _lib, engine, flatten_dev
    from tao_amodal_amd.synth import synth
    V, F, D = CONFIGS[a.config]
    V = a.videos or V
    dev = torch.device("cuda", 0)
    gt, dt = synth(seed=a.seed, V=V, F=F, C=a.cats, dets_per_frame=D)
    if a.level == "track":
        return track_level(a, gt, dt, dev, V)
    fl = flatten_dev.flatten_lvis(gt, dt, device=dev)
    dp = engine.DeviceProblem(fl, dev)
    ws = engine.Workspace(dp)
    engine.run_guarded(dp, ws, fl, upto="match", read_count=False)
    torch.cuda.synchronize()

    def timed(fn):
        return timed_calls(fn, a.warmup, a.reps)

    res = {"config": a.config, "videos": V, "rows": dp.n_dt, "ground_truths": dp.n_gt,
           "categories": dp.n_cat, "cells": dp.n_cells, "same_category_pairs": dp.n_iou}
    res["match_fused"] = timed(lambda: engine.stage_match(dp, ws))
    # the first call builds the per-image lists and runs the detail-mode match
    engine.stage_error_types(dp, ws, 0, a.bg_thr)
    torch.cuda.synchronize()
    res["match_with_match_gt"] = timed(
        lambda: engine.stage_match(dp, ws, match_gt=ws.err_match_gt))
    res["error_types"] = timed(lambda: engine.stage_error_types(dp, ws, 0, a.bg_thr))
    res["error_types_per_detection"] = timed(
        lambda: engine.stage_error_types(dp, ws, 0, a.bg_thr, per_detection=True))
    n_img, g_off, _, d_off, _ = dp.err_tabs
    g_cnt = (g_off[1:] - g_off[:-1]).long()
    d_cnt = (d_off[1:] - d_off[:-1]).long()
    res["images"] = n_img
    res["image_pairs"] = int((g_cnt * d_cnt).sum().item())
    res["max_gt_per_image"] = int(g_cnt.max().item())
    res["max_dt_per_image"] = int(d_cnt.max().item())
    _lib.kernel_timing(True)
    for _ in range(a.reps):
        engine.stage_error_types(dp, ws, 0, a.bg_thr)
    res["kernels_ms"] = {k: round(ms / n, 4) for k, (ms, n) in _lib.kernel_timings().items()}
    _lib.kernel_timing(False)
    res["dt_counts_by_type_range0"] = ws.err_dt_counts[0].sum(0).tolist()
    res["gt_counts_range0"] = ws.err_gt_counts[0].sum(0).tolist()
    if a.impact:
        # the first call allocates the link tables and the sweep's workspace
        engine.stage_error_impact(dp, ws, 0, a.bg_thr)
        torch.cuda.synchronize()
        res["error_types_links"] = timed(
            lambda: engine._error_pass(dp, ws, 0, a.bg_thr, dp.kind, per_detection=True,
                                       links=True))
        res["error_impact_links_and_sweep"] = timed(
            lambda: engine.stage_error_impact(dp, ws, 0, a.bg_thr))
        _lib.kernel_timing(True)
        for _ in range(a.reps):
            engine.stage_error_impact(dp, ws, 0, a.bg_thr)
        res["impact_kernels_ms"] = {k: round(ms / n, 4)
                                    for k, (ms, n) in _lib.kernel_timings().items()}
        _lib.kernel_timing(False)
        res["impact_sweep_kernels_ms"] = round(sum(
            v for k, v in res["impact_kernels_ms"].items() if k.startswith("imp_")), 4)
        res["impact_workspace_bytes"] = int(ws.imp_bytes)
        p = ws.imp_precision[..., 0].cpu().numpy()
        ap_ = [float(v[v > -1].mean()) if (v > -1).any() else -1.0 for v in p]
        res["fixes"] = list(_lib.ERROR_FIXES)
        res["ap_range0"] = [round(v, 6) for v in ap_]
        res["dap_range0"] = [round(v - ap_[0], 6) for v in ap_[1:]]
    if a.confusion:
        confusion(a, res, dp, ws, timed)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
