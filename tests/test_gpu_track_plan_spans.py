"""-m gpu: the span-aware 3D-IoU plan through the planned path.  Track pairs
without a common timeline position are kept out of the tasks and written as
+0.0 by the task launch's trailing workgroups, in every pass: the results are
the C oracle's bit for bit (compared as int64, so +0.0 and -0.0 differ),
whatever the IoU buffer held before the pass, in all three modes, on the inputs
of test_track_plan_spans_host.py."""
import copy

import numpy as np
import pytest

import boxpop
import orclib
import spanpop
from scorepop import same_values
from test_gpu_match_routes import _launches
from test_gpu_parity import _compare_with_oracle, _drop_frames
from tao_amodal_amd import flatten as fl
from tao_amodal_amd.synth import synth

pytestmark = pytest.mark.gpu

MODES = ("3d_iou", "avg_iou", "imagenetvid")


def _bits_equal(got, want):
    """Bit for bit (+0.0 is not -0.0); a computed NaN (0 / 0 of two tracks
    without frames) where the oracle has one."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if not np.isnan(want).any():
        return np.array_equal(got.view(np.int64), want.view(np.int64))
    return same_values(got, want)


def _stage(dp, ws, fill):
    import torch
    from tao_amodal_amd import engine
    ws.iou.fill_(fill)
    with _launches() as names:
        engine.stage_track_iou(dp, ws)
    torch.cuda.synchronize()
    return ws.iou[:dp.n_iou].cpu().numpy(), int(ws.pair_frames.item()), names


def _check_stage(f, planned=True):
    """stage_track_iou in every mode against orclib.track_iou: a first pass over
    a buffer of NaNs, a second over a buffer of ones (in mode 0 the instance
    that no longer counts frames), then the plan-less kernel.  Returns the
    number of zero-list entries of the plan."""
    from tao_amodal_amd import engine
    n_zero = 0
    for mode in MODES:
        want, want_pairs = orclib.track_iou(f, mode)
        dp = engine.DeviceProblem(f, iou_3d_type=mode)
        assert (dp.t["tasks"] is not None) == planned, mode
        assert (dp.t["zero_out"] is not None) == planned, mode
        ws = engine.Workspace(dp)
        for fill in (float("nan"), 1.0):
            iou, pairs, names = _stage(dp, ws, fill)
            assert _bits_equal(iou, want), (mode, fill)
            assert pairs == want_pairs, (mode, fill)
            assert ("track_iou_task_kernel" in names) == planned, names
            assert ("track_iou_kernel" in names) == (not planned), names
        if planned:
            n_zero = int(dp.t["zero_out"].numel())
            meta = engine.track_meta(f)[0]
            assert np.array_equal(np.sort(dp.t["zero_out"].cpu().numpy()),
                                  spanpop.zero_places(f, meta))
            assert (want[spanpop.zero_places(f, meta)].view(np.int64) == 0).all()   # +0.0
            dp.t["tasks"] = None
            iou, pairs, names = _stage(dp, engine.Workspace(dp), float("nan"))
            assert "track_iou_kernel" in names and "track_iou_task_kernel" not in names
            assert _bits_equal(iou, want) and pairs == want_pairs, mode
    return n_zero


def _check_evaluation(f):
    """evaluate_flat in every mode against the oracle: IoUs as bit patterns,
    pair_frames, precision and recall."""
    from tao_amodal_amd import engine
    for mode in MODES:
        want = orclib.run_flat(f, iou_3d_type=mode)
        got = engine.evaluate_flat(f, detail=True, iou_3d_type=mode)
        assert _bits_equal(got["iou"], want["iou"]), mode
        assert got["pairs"] == want["pairs"], mode
        assert np.array_equal(got["matched"], want["matched"]), mode
        assert np.array_equal(got["precision"], want["precision"]), mode
        assert np.array_equal(got["recall"], want["recall"]), mode


@pytest.mark.parametrize("name", list(spanpop.HAND_CELLS))
def test_hand_built_cells(name):
    f = spanpop.span_flat(spanpop.HAND_CELLS[name], holes=0.3)
    n_zero = _check_stage(f)
    _check_evaluation(f)
    want = {"touching": 0, "adjacent": 2, "nested": 0}.get(name)
    assert want is None or n_zero == want


@pytest.mark.parametrize("which", ["gt", "dt", "both"])
def test_tracks_without_frames_stay_in_the_tasks(which):
    """A track emptied in the flattened tables: its pairs are no zero pairs
    (two empty tracks: the reference's 0 / 0 in avg_iou and imagenetvid)."""
    f = spanpop.span_flat(spanpop.HAND_CELLS["no_frames"])
    if which in ("gt", "both"):
        f = spanpop.without_frames(f, "gt", 0)
    if which in ("dt", "both"):
        f = spanpop.without_frames(f, "dt", 0)
    if which == "both":
        assert np.isnan(orclib.track_iou(f, "avg_iou")[0][0])
    assert _check_stage(f) > 0


@pytest.mark.parametrize("n_gt", [33, 32, 63, 64, 96])
def test_forty_detections_at_the_gt_block_edges(n_gt):
    f = spanpop.span_flat([spanpop.big_cell(n_gt)])
    assert np.diff(f.cell_gt_off).tolist() == [n_gt]
    # (more entries than one trailing workgroup's threads: the strided loop)
    assert _check_stage(f) > 192
    _check_evaluation(f)


def test_a_cell_that_spills_over_several_tasks():
    f = spanpop.span_flat([spanpop.spill_cell(), spanpop.MIXED], holes=0.2)
    assert _check_stage(f) > 192
    _check_evaluation(f)


def test_no_zero_pair_at_all():
    """No trailing workgroup: the launch of the plan that holds every pair."""
    f = spanpop.span_flat(spanpop.no_zero_cells())
    assert _check_stage(f) == 0
    _check_evaluation(f)


def test_every_pair_a_zero_pair_drops_the_plan():
    f = spanpop.span_flat(spanpop.ALL_ZERO)
    assert _check_stage(f, planned=False) == 0
    _check_evaluation(f)
    want, _ = orclib.track_iou(f)
    assert (want.view(np.int64) == 0).all()


@pytest.mark.parametrize("seed,V,F,G,dpf", [(32, 2, 200, 40, 40), (34, 2, 200, 14, 40),
                                            (33, 1, 200, 8, 40)])
def test_synthetic_sets(seed, V, F, G, dpf):
    gt, dt = synth(seed=seed, V=V, F=F, C=6, dets_per_frame=dpf,
                   gt_tracks_per_video=G, n_present=2, n_neg=1)
    for holes in (False, True):
        if holes:
            gt, dt = _drop_frames(gt, dt, seed)
        dt.track_id, _ = fl.make_track_ids_unique(dt)
        f = fl.flatten_tao(gt, dt)
        # (seed 32: 1947 entries, two trailing workgroups; the others one)
        assert _check_stage(f) > 150
    _compare_with_oracle(f, _engine().evaluate_flat(f, detail=True))


def _engine():
    from tao_amodal_amd import engine
    return engine


# ---------------------------------------------------------------------------
# box populations in zero pairs and in kept pairs
# ---------------------------------------------------------------------------
def _odd_tracks(f, kind):
    """Per track (detections, then GTs): holds a box of the population's kind."""
    def odd(b):
        with np.errstate(all="ignore"):
            area = b[:, 2] * b[:, 3]
        if kind == "flipped":
            return (b[:, 2] < 0) & (b[:, 3] < 0)
        if kind == "scales":
            return np.isinf(area) | (np.abs(b).max(1) > 1e100)
        return np.abs(b).max(1) > 9e299
    out = []
    for side in ("dt", "gt"):
        off = np.asarray(f[side + "_frame_off"])
        o = odd(np.asarray(f[side + "_frame_box"], dtype=np.float64))
        c = np.concatenate([[0], np.cumsum(o)])
        out.append(c[off[1:]] - c[off[:-1]] > 0)
    return np.concatenate(out)


@pytest.mark.parametrize("kind", ["flipped", "scales", "near_far"])
def test_box_populations_in_zero_pairs_and_kept_pairs(kind):
    """w < 0 and h < 0 together, areas that overflow to +-inf (a GT keeps such
    a box), coordinates near +-9.9e299 (inside the task kernel's domain): the
    zero rule holds whatever the boxes are (mode 0: 0 / u, or the u > 0 test's
    0.0 for u = inf, NaN or negative), so the planned result is the oracle's
    and the plan-less kernel's, in pairs on the zero list and in the tasks."""
    from tao_amodal_amd import engine
    cells = spanpop.HAND_CELLS["everything"] + [spanpop.big_cell(33, n_dt=20)]
    gt, dt = spanpop.span_columns(cells, holes=0.2)
    rng = np.random.default_rng([0x5ba4, len(kind)])
    if kind != "near_far":
        boxpop.implant(gt, dt, kind, rng, gt_share=0.3, dt_share=0.15)
    f = fl.flatten_tao(gt, dt)
    if kind == "near_far":
        f = copy.copy(f)
        for side in ("dt", "gt"):
            box = np.array(f[side + "_frame_box"], dtype=np.float64)
            rows = np.flatnonzero(rng.random(len(box)) < 0.1)
            box[rows, rng.integers(0, 2, len(rows))] = rng.choice(
                [9.9e299, -9.9e299, np.nextafter(1e300, 0)], len(rows))
            f[side + "_frame_box"] = box
    meta = engine.track_meta(f)[0]
    odd = _odd_tracks(f, kind)
    _, pd, pg = spanpop.pair_tracks(f)
    pair_odd = odd[pd] | odd[int(f.cell_dt_off[-1]) + pg]
    zero = np.zeros(len(pd), bool)
    zero[spanpop.zero_places(f, meta)] = True
    assert (pair_odd & zero).sum() >= 10 and (pair_odd & ~zero).sum() >= 10
    assert _check_stage(f) > 0
    for mode in MODES:
        want = orclib.run_flat(f, iou_3d_type=mode)
        got = engine.evaluate_flat(f, detail=True, iou_3d_type=mode)
        assert _bits_equal(got["iou"], want["iou"]), mode
        assert np.array_equal(got["precision"], want["precision"]), mode
        assert np.array_equal(got["recall"], want["recall"]), mode


@pytest.mark.parametrize("col,v", [(0, 1e300), (1, -1e300), (3, np.nan), (2, np.inf)])
def test_a_table_outside_the_domain_still_drops_the_plan(col, v):
    """Bit 1 of taoamd_track_pad's flag: no tasks and no zero list; the
    plan-less kernel computes every pair, zero pairs included."""
    f = spanpop.span_flat(spanpop.HAND_CELLS["everything"])
    g = copy.copy(f)
    box = np.array(f.gt_frame_box)
    box[3, col] = v
    g.gt_frame_box = box
    assert _check_stage(g, planned=False) == 0


# ---------------------------------------------------------------------------
# decimal coordinates: the frame-order guard reads the zeros
# ---------------------------------------------------------------------------
def test_decimal_set_with_the_guard_active(monkeypatch):
    """A 2-video decimal set: the guard lists pairs from the IoU matrix the
    planned pass wrote (its zeros are skipped as before); the evaluation is the
    oracle's and the guard lists as many pairs as under the plan that keeps
    every pair in a task."""
    from tao_amodal_amd import engine
    gt, dt = synth(seed=41, V=2, F=60, C=6, dets_per_frame=12, gt_tracks_per_video=6,
                   n_present=2, n_neg=1, decimal=True)
    dt.track_id, _ = fl.make_track_ids_unique(dt)
    f = fl.flatten_tao(gt, dt)
    dp = engine.DeviceProblem(f)
    assert dp.guard_active() and dp.t["tasks"] is not None and dp.t["zero_out"].numel() > 0
    got = engine.evaluate_flat(f, detail=True)
    _compare_with_oracle(f, got)
    monkeypatch.setattr(engine, "track_iou_plan_spans", lambda flat, meta:
                        engine.track_iou_plan(flat, meta) + (np.zeros(0, np.int64),))
    dp = engine.DeviceProblem(f)
    assert dp.t["zero_out"].numel() == 0
    old = engine.evaluate_flat(f, detail=True)
    assert got["near_threshold_pairs"] == old["near_threshold_pairs"]
    assert np.array_equal(got["iou"].view(np.int64), old["iou"].view(np.int64))
