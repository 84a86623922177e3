"""-m gpu: the greedy match's compiled variants on rule-dense cells.

The match is one host entry (taoamd_match) over seven kernel instances that
the launch plan (engine.match_plan) picks by cell size: match_group_kernel
(runs of cells of <= 8 GTs; closed form or sequential greedy inside),
match_kernel (every other cell of <= 64 GTs) and match_big_kernel (up to
TAOAMD_MAX_GT_PER_CELL).  fixtures.rule_cells puts the reference's match rules
-- IoU ties across the ignore order, IoUs exactly on every threshold and at 1,
ignored-best candidates, range bounds, equal scores, id sentinels, detections
that do not consume -- into cells of a chosen size; every run here must equal
the C oracle (pinned to the reference by the F9 goldens) bit for bit, and each
case checks from the launch names which kernels did the work."""
import contextlib
import copy
import functools
import os
import sys

import numpy as np
import pytest

import orclib
from test_gpu_parity import _compare_with_oracle
from tao_amodal_amd import _lib
from tao_amodal_amd import flatten as fl
from tao_amodal_amd.columns import DTColumns, GTColumns

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import fixtures  # noqa: E402

pytestmark = pytest.mark.gpu

MATCH_KERNELS = {"match_group_kernel", "match_kernel", "match_big_kernel"}
# one video per entry; the track-level cell holds that many GT tracks, the
# image-level cell of its first frame that many GTs
SIZE_CLASSES = {
    "group": [8, 6, 8, 5, 7, 8, 3, 8, 4, 8, 2, 8],
    "single": [12, 40, 64, 9],
    "big": [65, 96, 97, 130],
}


@functools.lru_cache(maxsize=None)
def _inputs(sizes):
    return fixtures.rule_cells(list(sizes), hidden_in=0)


def _flat(level, sizes):
    gtj, predj = _inputs(tuple(sizes))
    gt, dt = GTColumns.from_json(gtj), DTColumns.from_json(predj)
    if level == "lvis":
        return fl.flatten_lvis(gt, dt)
    dt.track_id, _ = fl.make_track_ids_unique(dt)
    return fl.flatten_tao(gt, dt)


@contextlib.contextmanager
def _launches():
    """Names (without the evaluator label) of the kernels launched inside."""
    import torch
    names = set()
    _lib.kernel_timing(True)
    try:
        _lib.kernel_timings()                   # forget earlier launches
        yield names
        torch.cuda.synchronize()
        names.update(k.rsplit(":", 1)[-1] for k in _lib.kernel_timings())
    finally:
        _lib.kernel_timing(False)


def _routes(dp, f):
    """The match kernels the problem's plan gives work to (match_kernel is
    launched for every plan with singles: its big cells return at once)."""
    G = np.diff(f.cell_gt_off)
    s = dp.singles_host
    out = set()
    if dp.n_groups:
        out.add("match_group_kernel")
    if len(s):
        out.add("match_kernel")
        if G[s].max() > 64:
            out.add("match_big_kernel")
    return out


def _multi_candidate_cells(f, iou):
    """Per cell: does some detection reach the lowest threshold with two GTs
    (the group kernel's sequential path) -- from the oracle's IoUs."""
    thr0 = orclib.thresholds()[0][0]
    off = orclib.iou_offsets(f)
    out = np.zeros(f.n_cells, bool)
    for c in range(f.n_cells):
        D = f.cell_dt_off[c + 1] - f.cell_dt_off[c]
        G = f.cell_gt_off[c + 1] - f.cell_gt_off[c]
        if D and G:
            m = iou[off[c]:off[c + 1]].reshape(D, G)
            out[c] = ((m >= thr0).sum(axis=1) >= 2).any()
    return out


def _check_plan(size_class, dp, f):
    from tao_amodal_amd import engine
    G = np.diff(f.cell_gt_off)
    s = dp.singles_host
    assert dp.max_g == G.max()
    if size_class == "group":
        assert dp.n_groups > 0 and dp.n_singles == 0 and dp.max_g <= 8
        # closed form and sequential greedy side by side in one run
        groups, _ = engine.match_plan(f.cell_dt_off, f.cell_gt_off)
        multi = _multi_candidate_cells(f, orclib.run_flat(f)["iou"])
        mixed = [bool(multi[a:b].any() and not multi[a:b].all()) for a, b in groups]
        assert sum(mixed) >= 2, mixed
    elif size_class == "single":
        assert dp.n_singles > 0 and 8 < dp.max_g <= 64
        assert {12, 40, 64, 9} <= set(G[s].tolist())
    else:
        assert {65, 96, 97, 130} <= set(G[s].tolist())


@pytest.mark.parametrize("level", ["lvis", "tao"])
@pytest.mark.parametrize("size_class", list(SIZE_CLASSES))
def test_every_route_equals_the_oracle_on_rule_dense_cells(level, size_class):
    """evaluate_flat with and without detail (image level: the group kernel's
    <true, false> instance, IoUs fused) and the production layout (image
    level: the FAST <true, true> instance), each equal to the oracle."""
    import torch
    from tao_amodal_amd import engine
    f = _flat(level, SIZE_CLASSES[size_class])
    dp = engine.DeviceProblem(f)
    _check_plan(size_class, dp, f)
    want_routes = _routes(dp, f)
    assert {"group": "match_group_kernel", "single": "match_kernel",
            "big": "match_big_kernel"}[size_class] in want_routes
    for detail in (True, False):
        with _launches() as names:
            got = engine.evaluate_flat(f, detail=detail)
        assert names & MATCH_KERNELS == want_routes, (detail, names)
        _compare_with_oracle(f, got, detail=detail)
    # production path: the workspace the CLI and the class API allocate
    want = orclib.run_flat(f, detail=False)
    ws = engine.Workspace(dp)
    assert ws.match_gt is None and (level == "tao") == (ws.dt_rng is not None)
    with _launches() as names:
        engine.run(dp, ws)
    assert names & MATCH_KERNELS == want_routes, names
    torch.cuda.synchronize()
    n = dp.n_dt
    dst = ws.dst[:n].long()
    assert np.array_equal(ws.gt_rng[:dp.n_gt].cpu().numpy().view(np.uint32),
                          want["gt_rng"])
    assert np.array_equal(ws.num_gt.cpu().numpy(), want["num_gt"])
    assert np.array_equal(ws.matched[:n][dst].cpu().numpy().view(np.uint64),
                          want["matched"])
    assert np.array_equal(ws.ignored[:n][dst].cpu().numpy().view(np.uint64),
                          want["ignored"])
    assert np.array_equal(ws.precision.cpu().numpy(), want["precision"])
    assert np.array_equal(ws.recall.cpu().numpy(), want["recall"])


@pytest.mark.parametrize("level", ["lvis", "tao"])
def test_forced_singles_equal_the_grouped_run(level, monkeypatch):
    """The group-sized problem with a plan of caps 0 -- every cell a single --
    runs through match_kernel alone and gives the grouped run's rows."""
    from tao_amodal_amd import engine
    f = _flat(level, SIZE_CLASSES["group"])
    grouped = engine.evaluate_flat(f, detail=True)
    plan = engine.match_plan
    monkeypatch.setattr(engine, "match_plan",
                        lambda d_off, g_off, *a, **k: plan(d_off, g_off, 0, 0, 0))
    dp = engine.DeviceProblem(f)
    assert dp.n_groups == 0 and dp.n_singles == int((np.diff(f.cell_dt_off) > 0).sum())
    for detail in (True, False):
        with _launches() as names:
            got = engine.evaluate_flat(f, detail=detail)
        assert names & MATCH_KERNELS == {"match_kernel"}, names
        _compare_with_oracle(f, got, detail=detail)
        for k in ("matched", "ignored", "precision", "recall"):
            assert np.array_equal(got[k], grouped[k]), k
        if detail:
            assert np.array_equal(got["match_gt"], grouped["match_gt"])


def _with_rect_masks(gtj):
    g = copy.deepcopy(gtj)
    for im in g["images"]:
        im["height"] = im["width"] = 1024
    for a in g["annotations"]:
        x, y, w, h = a["bbox"]
        a["segmentation"] = [[x, y, x, y + h, x + w, y + h, x + w, y]]
    return g


@pytest.mark.parametrize("size_class", list(SIZE_CLASSES))
def test_image_level_segm_on_rectangles_equals_the_boxes(size_class):
    """LVISEval(iou_type="segm") on rectangle masks of the same integer boxes:
    the IoUs come from the run-length kernel, so the match runs its non-fused
    image-level instances -- and must give the bbox run's numbers."""
    from tao_amodal_amd.evaluation.lvis_amodal import LVIS, LVISEval, LVISResults
    gtj, predj = _inputs(tuple(SIZE_CLASSES[size_class]))
    f = _flat("lvis", SIZE_CLASSES[size_class])
    want = orclib.run_flat(f, detail=False)
    out = {}
    for kind in ("bbox", "segm"):
        gt = LVIS(_with_rect_masks(gtj))
        ev = LVISEval(gt, LVISResults(gt, copy.deepcopy(predj)), kind)
        with _launches() as names:
            ev.evaluate()
            ev.accumulate()
        dp = ev._run.dp
        assert dp.mask_iou == (kind == "segm")
        assert names & MATCH_KERNELS == _routes(dp, f), (kind, names)
        if kind == "segm":
            assert "rle_iou_kernel" in names, names
        out[kind] = ev
    for ev in out.values():
        assert np.array_equal(ev.eval["precision"], want["precision"])
        assert np.array_equal(ev.eval["recall"], want["recall"])


@pytest.mark.parametrize("level", ["lvis", "tao"])
def test_cell_of_3072_ground_truths(level):
    """The largest cell match_big_kernel holds in LDS."""
    from tao_amodal_amd import engine
    f = _flat(level, [_lib.MAX_GT_PER_CELL])
    dp = engine.DeviceProblem(f)
    assert dp.max_g == _lib.MAX_GT_PER_CELL == 3072
    with _launches() as names:
        got = engine.evaluate_flat(f, detail=True)
    assert names & MATCH_KERNELS == _routes(dp, f)
    assert "match_big_kernel" in names
    _compare_with_oracle(f, got)


@pytest.mark.parametrize("level", ["lvis", "tao"])
def test_cell_of_3073_ground_truths_is_refused_before_any_launch(level):
    from tao_amodal_amd import engine
    f = _flat(level, [_lib.MAX_GT_PER_CELL + 1])
    assert np.diff(f.cell_gt_off).max() == 3073
    with _launches() as names:
        with pytest.raises(_lib.TaoAmdError, match="3073"):
            engine.DeviceProblem(f)
    assert names == set()
