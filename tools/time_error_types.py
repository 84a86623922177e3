#!/usr/bin/env python
"""Measurement of the image-level error breakdown (taoamd_error_types) on the
synthetic configurations of bench.py, with HIP events:

    python tools/time_error_types.py [--config 3s] [--reps 20] [--warmup 3]

Times, on the image level's tables of that configuration, each alone on an idle
stream: the fused match as a benchmark step runs it (the yardstick), the
detail-mode match that produces match_gt (existing code the breakdown depends
on), and the breakdown itself with and without the per-detection table; lists
the breakdown's kernels and the pair counts that bound it (an image's
detections x ALL its ground truths against the match's same-category pairs).
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CONFIGS = {"2": (200, 300, 50), "3s": (2000, 300, 50), "5s": (10000, 1, 1000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="3s")
    ap.add_argument("--videos", type=int, default=None)
    ap.add_argument("--cats", type=int, default=1203)
    ap.add_argument("--seed", type=int, default=20240807)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bg-thr", type=float, default=0.1)
    a = ap.parse_args()
    import torch
    from tao_amodal_amd import _lib, engine, flatten_dev
    from tao_amodal_amd.synth import synth
    V, F, D = CONFIGS[a.config]
    V = a.videos or V
    dev = torch.device("cuda", 0)
    gt, dt = synth(seed=a.seed, V=V, F=F, C=a.cats, dets_per_frame=D)
    fl = flatten_dev.flatten_lvis(gt, dt, device=dev)
    dp = engine.DeviceProblem(fl, dev)
    ws = engine.Workspace(dp)
    engine.run_guarded(dp, ws, fl, upto="match", read_count=False)
    torch.cuda.synchronize()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return {"min_ms": round(min(out), 4), "median_ms": round(float(np.median(out)), 4),
                "max_ms": round(max(out), 4)}

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
    n_img, g_off, _, d_off, _, _ = dp.err_tabs
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
    print(json.dumps(res))


if __name__ == "__main__":
    main()
