#!/usr/bin/env python
"""Measurement of TaoEval(iou_type="segm"): the 3D mask IoU of track pairs on
the GPU (taoamd_track_mask_iou) next to the plain-Python restatement
(tests/track_segm_ref.py, one host core) on a sample of the same cells.

    python tools/bench_track_segm.py [--videos 200] [--frames 60]

Synthetic workload, seeded: one cell per video with --gts GT tracks (a
contiguous stretch of 20..frames frames each) and --dets detection tracks per
GT track that follow it (a frame dropped now and then, the box jittered);
1280 x 720 frames, every mask a polygon of 8-16 vertices around its box.  The
kernel is timed with device events after warm-up.  Prints one JSON line: the
rate in (pair, shared frame) items per second and the algorithmic bytes (every
run read once, every IoU written once) over kernel time."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))


def poly(rng, box, n):
    x, y, w, h = box
    cx, cy = x + w / 2, y + h / 2
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(0.8, 1.0, n)
    return np.c_[cx + rad * w / 2 * np.cos(ang), cy + rad * h / 2 * np.sin(ang)].ravel().tolist()


def workload(a):
    """(cells_d, cells_g, per side: (frame_off, frame_pos, polygon items))"""
    H, W = 720, 1280
    rng = np.random.default_rng(a.seed)
    side = {"dt": ([], [], []), "gt": ([], [], [])}     # lengths, positions, items
    for _ in range(a.videos):
        gts = []
        for _ in range(a.gts):
            n = int(rng.integers(min(20, a.frames), a.frames + 1))
            f0 = int(rng.integers(0, a.frames - n + 1))
            b = np.r_[rng.uniform(0, W - 400), rng.uniform(0, H - 300),
                      rng.uniform(40, 400), rng.uniform(40, 300)]
            v = rng.uniform(-4, 4, 2)
            boxes = {f0 + k: b + np.r_[v * k, 0, 0] for k in range(n)}
            gts.append(boxes)
            lens, pos, items = side["gt"]
            lens.append(n)
            for p, bb in boxes.items():
                pos.append(p)
                items.append(([poly(rng, bb, int(rng.integers(8, 17)))], H, W))
        for g in range(a.gts * a.dets):
            boxes = gts[g % a.gts]
            keep = [p for p in boxes if rng.random() > 0.1] or [min(boxes)]
            lens, pos, items = side["dt"]
            lens.append(len(keep))
            for p in keep:
                bb = boxes[p] + rng.uniform(-12, 12, 4)
                bb[2:] = np.maximum(bb[2:], 8)
                pos.append(p)
                items.append(([poly(rng, bb, int(rng.integers(8, 17)))], H, W))
    cells_d = np.full(a.videos, a.gts * a.dets, np.int64)
    cells_g = np.full(a.videos, a.gts, np.int64)
    return cells_d, cells_g, side


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=200)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--gts", type=int, default=4)
    ap.add_argument("--dets", type=int, default=2, help="detection tracks per GT track")
    ap.add_argument("--mode", default="3d_iou", choices=["3d_iou", "avg_iou", "imagenetvid"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-cells", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch
    from tao_amodal_amd import _lib
    from tao_amodal_amd.masks import MaskBatch
    cells_d, cells_g, side = workload(a)
    t0 = time.perf_counter()
    tabs = {}
    for s in ("dt", "gt"):
        lens, pos, items = side[s]
        b = MaskBatch()
        b.add_many(items)
        tabs[s] = (np.r_[0, np.cumsum(lens)].astype(np.int32), np.asarray(pos, np.int32),
                   b.arrays())
        b.close()
    t_build = time.perf_counter() - t0
    d_off = np.r_[0, np.cumsum(cells_d)].astype(np.int32)
    g_off = np.r_[0, np.cumsum(cells_g)].astype(np.int32)
    i_off = np.r_[0, np.cumsum(cells_d * cells_g)].astype(np.int64)
    n_pairs = int(i_off[-1])
    dev = "cuda"
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    head = [t(d_off), t(g_off), t(i_off)]
    keep, args = [], []
    for s in ("dt", "gt"):
        off, pos, m = tabs[s]
        xs = [t(off), t(pos), t(m.off), t(m.counts.view(np.int32)), t(m.hw)]
        keep += xs
        args += [xs[0].data_ptr(), xs[1].data_ptr(), len(m), int(m.off[-1])] + \
            [x.data_ptr() for x in xs[2:]]
    out = torch.empty(n_pairs, dtype=torch.float64, device=dev)
    pf = torch.zeros(1, dtype=torch.int64, device=dev)
    lib = _lib.load()
    dt, gt = tabs["dt"][2], tabs["gt"][2]
    nb = lib.taoamd_track_mask_iou_workspace(len(dt), int(dt.off[-1]), len(gt), int(gt.off[-1]))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    mode = ["3d_iou", "avg_iou", "imagenetvid"].index(a.mode)

    def launch():
        assert lib.taoamd_track_mask_iou(
            len(cells_d), *[x.data_ptr() for x in head], n_pairs, *args, mode,
            out.data_ptr(), pf.data_ptr(), ws.data_ptr(), nb, st) == 0
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(a.reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    got = out.cpu().numpy()
    items = int(pf.item())
    once = (len(dt.counts) + len(gt.counts)) * 4 + n_pairs * 8
    # the restatement on a sample of the cells, one core
    import track_segm_ref as ref
    masks = {s: [tabs[s][2].mask(i) for i in range(len(tabs[s][2]))] for s in ("dt", "gt")}
    trk = {s: ref.tracks_of(tabs[s][0], tabs[s][1], masks[s]) for s in ("dt", "gt")}
    cells = list(range(0, len(cells_d), max(1, len(cells_d) // a.cpu_cells)))[:a.cpu_cells]
    t0 = time.perf_counter()
    ok, cpu_items = True, 0
    for c in cells:
        for d in range(d_off[c], d_off[c + 1]):
            for g in range(g_off[c], g_off[c + 1]):
                v = ref.track_iou(trk["dt"][d], trk["gt"][g], a.mode)
                cpu_items += ref.shared_frames(trk["dt"][d], trk["gt"][g])
                k = i_off[c] + (d - d_off[c]) * cells_g[c] + (g - g_off[c])
                ok = ok and v == got[k]
    t_cpu = time.perf_counter() - t0
    print(json.dumps({
        "metric": "track-level mask IoU throughput", "unit": "Mitem/s",
        "value": round(items / ms / 1e3, 2), "ms_per_launch": round(ms, 4),
        "items": items, "pairs": n_pairs, "mode": a.mode,
        "runs_per_mask": round(float((len(dt.counts) + len(gt.counts)) / (len(dt) + len(gt))), 1),
        "roofline": {"bound": "hbm", "unit": "GB/s",
                     "achieved": round(once / ms / 1e6, 1), "peak": 8000,
                     "frac": round(once / ms / 1e6 / 8000, 4), "bytes_once": once},
        "cpu_baseline": {"kind": "restatement (tests/track_segm_ref.py)",
                         "value": round(cpu_items / t_cpu / 1e6, 5), "unit": "Mitem/s",
                         "cores": 1, "sample": "%d cells (%d items)" % (len(cells), cpu_items),
                         "equal_to_gpu": bool(ok)},
        "host_mask_build_s": round(t_build, 2),
        "config": {"workload": "%d videos x %d frames, %d GT tracks x %d det tracks each, "
                               "1280x720 polygons" % (a.videos, a.frames, a.gts, a.dets)},
    }))


if __name__ == "__main__":
    main()
