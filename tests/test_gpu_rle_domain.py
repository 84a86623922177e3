"""The mask IoU kernels on the run-length population of tests/rlepop.py --
every blocking edge of csrc/rle_walk.hpp, rle_iou.hip and track_mask_iou.hip,
and the pixels at which the reference stops counting -- against the oracle
(oracle/rle.py, tests/track_segm_ref.py; both pinned to the reference C on
this population by test_rle_domain_host.py).  The drivers are those of
test_gpu_masks.py and test_gpu_track_segm.py, guarded workspace included."""
import copy
import functools

import numpy as np
import pytest

import rlepop
import test_gpu_masks as image_level
import test_gpu_track_segm as track_level
import track_segm_ref as ref
import wsguard
from oracle import pyoracle, rle
from tao_amodal_amd.masks import MaskBatch

pytestmark = pytest.mark.gpu

MODES = track_level.MODES


# ------------------------------------------------------------- image level
@functools.lru_cache(maxsize=None)
def _cells(kind):
    """The cells of a kind and their IoU matrices by the oracle.  The pairs of
    a pair kind are dealt to cells of up to 3 x 3, frame size by frame size, so
    that partners and strangers meet."""
    if kind == "cells":
        cells = rlepop.cells()[0]
    else:
        cells, pairs = [], rlepop.pairs_of(kind)[0]
        for k in range(0, len(pairs), 3):
            group = [p for p in pairs[k:k + 3] if p[0]["h"] == pairs[k][0]["h"]]
            cells.append(([d for d, _ in group], [g for _, g in group]))
    return cells, [rle.iou_matrix(dts, gts) for dts, gts in cells]


def _arrays(masks):
    b = MaskBatch()
    for m in masks:
        b.add({"size": [m["h"], m["w"]], "counts": m["counts"]}, 0, 0)
    a = b.arrays()
    b.close()
    return a


def _check_cells(kind):
    cells, want = _cells(kind)
    dt = _arrays([m for dts, _ in cells for m in dts])
    gt = _arrays([m for _, gts in cells for m in gts])
    cells_d, cells_g = [len(d) for d, _ in cells], [len(g) for _, g in cells]
    got, off = image_level._device_iou(cells_d, cells_g, dt, gt)
    for c, (D, G) in enumerate(zip(cells_d, cells_g)):
        if D and G:
            mine = got[off[c]:off[c + 1]].reshape(D, G)
            assert np.array_equal(mine, want[c]), (kind, c, np.argwhere(mine != want[c])[:4])
    return got, off


@pytest.mark.parametrize("kind", rlepop.PAIR_KINDS + ("cells",))
def test_rle_iou_kernel_equals_the_oracle(kind):
    _check_cells(kind)


def test_rle_iou_kernel_stops_where_the_reference_stops():
    """The three pairs of the stop rule's table, on a 2 x 3 frame."""
    masks = [[rlepop.mask(2, 3, c) for c in side] for side in zip(*rlepop.TABLE_ROWS)]
    got, _ = image_level._device_iou([1, 1, 1], [1, 1, 1], _arrays(masks[0]), _arrays(masks[1]))
    assert got.tolist() == [0.0, 1.0, 0.0]


@pytest.mark.parametrize("kind", ["empty_runs", "big_frames", "cells"])
def test_rle_iou_with_the_workspace_base_moved_by_8_bytes(kind, monkeypatch):
    monkeypatch.setattr(wsguard, "SHIFT", 8)
    _check_cells(kind)


# ------------------------------------------------------------- track level
_TERMS = {}          # (id(d_t), id(g_t)) -> (i_t, u_t): the population's masks live on


@functools.lru_cache(maxsize=None)
def _problems():
    """rlepop.tracks(), and every pair kind as tracks of up to 8 frames: frame
    t of a detection track is the d of a pair, of its ground-truth track the g."""
    probs = list(rlepop.tracks()[0])
    for kind in rlepop.PAIR_KINDS:
        pairs = rlepop.pairs_of(kind)[0]
        probs.append([([{t: d for t, (d, _) in enumerate(pairs[k:k + 8])}],
                       [{t: g for t, (_, g) in enumerate(pairs[k:k + 8])}])
                      for k in range(0, len(pairs), 8)])
    return probs


def _check_tracks(prob):
    cells_d, cells_g = [len(d) for d, _ in prob], [len(g) for _, g in prob]
    dts = [t for d, _ in prob for t in d]
    gts = [t for _, g in prob for t in g]
    f, sides = track_level._tables(cells_d, cells_g, dts, gts)
    items = sum(ref.shared_frames(d, g) for ds, gs in prob for d in ds for g in gs)
    for mode in MODES:
        got, pairs = track_level._device_iou(f, sides, mode)
        want = ref.cell_ious(f, dts, gts, mode, _TERMS)
        assert got.shape == want.shape
        bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
        assert len(bad) == 0, (mode, bad[:5], got[bad[:5]], want[bad[:5]])
        assert pairs == items, mode


@pytest.mark.parametrize("which", range(3 + len(rlepop.PAIR_KINDS)))
def test_track_mask_iou_kernel_equals_the_restatement(which):
    _check_tracks(_problems()[which])


def test_track_mask_iou_kernel_stops_where_the_reference_stops():
    """The table's pairs give (i_t, u_t) = (0, 0), (4, 4) and (0, 2); a second
    frame with (1, 4) makes them visible in every mode."""
    second = (rlepop.mask(2, 3, [2, 4]), rlepop.mask(2, 3, [5, 1]))
    assert ref.frame_terms(*second) == (1, 4)
    prob = [([{0: rlepop.mask(2, 3, a), 1: second[0]}], [{0: rlepop.mask(2, 3, b), 1: second[1]}])
            for a, b in rlepop.TABLE_ROWS]
    cells_d = cells_g = [1, 1, 1]
    dts, gts = [d[0] for d, _ in prob], [g[0] for _, g in prob]
    f, sides = track_level._tables(cells_d, cells_g, dts, gts)
    want = {"3d_iou": [1 / 4, 5 / 8, 1 / 6], "avg_iou": [(0 + 1 / 4) / 2, (1 + 1 / 4) / 2, 1 / 8],
            "imagenetvid": [0.0, 0.5, 0.0]}
    for mode in MODES:
        got, pairs = track_level._device_iou(f, sides, mode)
        assert got.tolist() == want[mode] and pairs == 6, mode
        assert got.tolist() == ref.cell_ious(f, dts, gts, mode).tolist()


def test_track_mask_iou_with_the_workspace_base_moved_by_8_bytes(monkeypatch):
    monkeypatch.setattr(wsguard, "SHIFT", 8)
    for which in (2, 6):                 # the five-pair problem, empty_runs
        _check_tracks(_problems()[which])


# --------------------------------------------------------------- class API
def _empty_run_dataset(seed):
    """A small set whose segmentations are uncompressed run lists and
    compressed strings with empty runs inside, on both sides; every third
    prediction repeats its ground truth's list, empty runs and all, so that
    the pair stops at the splice."""
    g, preds = track_level._rect_dataset(seed, V=3, F=4, C=2, H=12, W=16)
    H, W = 12, 16
    by_image = {}

    def segm(box, k):
        c = rle.fr_bbox(box, H, W)["counts"]
        c = rlepop.splice(c, k % len(c)) if k % 4 else [0, 0] + c
        m = {"h": H, "w": W, "counts": c}
        return {"size": [H, W], "counts": c if k % 2 else rle.to_string(m)}, m
    for k, a in enumerate(g["annotations"]):
        a["segmentation"], m = segm(a["bbox"], k)
        by_image.setdefault((a["image_id"], a["category_id"]), []).append((a, m))
    stopped = 0
    for k, p in enumerate(preds):
        a, m = by_image[p["image_id"], p["category_id"]][0]
        if k % 3 == 0:
            p["bbox"] = list(a["bbox"])
            p["segmentation"] = copy.deepcopy(a["segmentation"])
            stopped += rlepop.stop_pixel(m["counts"], m["counts"]) < H * W
        else:
            p["segmentation"], _ = segm(p["bbox"], k + 1)
    assert stopped >= 3
    return g, preds


def test_lvis_eval_segm_with_empty_runs_equals_the_oracle():
    from tao_amodal_amd.evaluation.lvis_amodal import LVIS, LVISEval, LVISResults
    g, preds = _empty_run_dataset(5)
    want = pyoracle.lvis_eval(g, preds, iou_type="segm")
    gt = LVIS(copy.deepcopy(g))
    ev = LVISEval(gt, LVISResults(gt, copy.deepcopy(preds)), "segm")
    ev.run()
    seen = 0
    for key, cell in want["cells"].items():
        w = np.asarray(cell["ious"], dtype=float)
        if w.size:
            assert np.array_equal(np.asarray(ev.ious[key]).reshape(w.shape), w), key
            seen += w.size
    assert seen > 20
    assert np.array_equal(ev.eval["precision"], want["precision"])
    assert np.array_equal(ev.eval["recall"], want["recall"])


@pytest.mark.parametrize("mode", MODES)
def test_tao_eval_segm_with_empty_runs_equals_the_restatement(mode):
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval
    g, preds = _empty_run_dataset(6)
    gt = Tao(copy.deepcopy(g))
    ev = TaoEval(gt, copy.deepcopy(preds), iou_type="segm", iou_3d_type=mode)
    ev.run()
    f, want = track_level._ref_cells(gt, preds, True, mode)
    seen = 0
    for k in range(f.n_cells):
        vid, cat = int(f.vid_ids[f.cell_unit[k]]), int(f.cat_ids[f.cell_cat[k]])
        D = f.cell_dt_off[k + 1] - f.cell_dt_off[k]
        G = f.cell_gt_off[k + 1] - f.cell_gt_off[k]
        got = np.asarray(ev.ious[vid, cat], dtype=np.float64).reshape(D, G)
        w = want[f.cell_iou_off[k]:f.cell_iou_off[k + 1]].reshape(D, G)
        assert np.array_equal(got.view(np.int64), w.view(np.int64)), (vid, cat)
        seen += D * G
    assert seen == len(want) and seen > 10
