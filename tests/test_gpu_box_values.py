"""-m gpu: every IoU and match kernel, the device table build, the device JSON
reader and the error breakdown on box coordinates that are any double
(tests/boxpop.py: decimal boxes across the frame edge and exact copies, pairs
that touch or miss by one ulp, w < 0 and h < 0 together, magnitudes 1e-160 to
1e150, coordinates at and beyond +-1e300, NaN in three bit patterns, +-inf,
-0.0 and +-5e-324).

The contract ("Box coordinates: the domain") is the C oracle's,
pinned on the host to the reference's compiled bbIou and to its Python track
IoU in test_box_values_host.py.  IoUs are compared NaN where the oracle has
NaN (sign and payload are the machine's) and bit for bit elsewhere,
everything else with ==.  That each case holds the edge it is about is
asserted from the oracle's tables, never from what the device returned."""
import copy
import functools
import json
import os
import sys

import numpy as np
import pytest

import boxpop
import error_types_ref as ref
import orclib
from boxpop import KINDS
from goldenio import path
from scorepop import same_values
from test_gpu_match_routes import MATCH_KERNELS, _launches, _routes
from test_gpu_parity import _compare_with_oracle, _drop_frames
from tao_amodal_amd import _lib
from tao_amodal_amd import flatten as fl
from tao_amodal_amd.columns import DTColumns, GTColumns
from tao_amodal_amd.synth import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import fixtures  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("3d_iou", "avg_iou", "imagenetvid")


# ---------------------------------------------------------------------------
# taoamd_bb_iou and taoamd_bb_iou_host
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_bb_iou_entry_points_on_the_reference_golden(kind):
    """Both entry points on the boxes of golden/maskapi/bb_iou_domain.npz
    against the reference's compiled bbIou, and with an iscrowd column against
    the C oracle: v_min_f64 / v_max_f64 on NaN, +-inf, -0.0, subnormals, on
    sums that overflow and on products that underflow."""
    import torch
    from test_box_values_host import crowd_column
    lib = _lib.load()
    z = np.load(path("maskapi", "bb_iou_domain.npz"))
    dt, gt, want = z[kind + "_dt"], z[kind + "_gt"], z[kind + "_iou"]
    m, n = len(dt), len(gt)
    crowd = crowd_column(kind, n)
    d_dt, d_gt = torch.from_numpy(dt).cuda(), torch.from_numpy(gt).cuda()
    d_crowd = torch.from_numpy(crowd).cuda()
    for col, d_col, ref_iou in ((None, None, want), (crowd, d_crowd, orclib.bb_iou(dt, gt, crowd))):
        o = np.full(m * n, -7.0)
        _lib.check(lib.taoamd_bb_iou_host(dt.ctypes.data, gt.ctypes.data, m, n,
                                          None if col is None else col.ctypes.data,
                                          o.ctypes.data), "bb_iou_host")
        assert same_values(o.reshape((m, n), order="F"), ref_iou)
        d_o = torch.full((m * n,), -7.0, dtype=torch.float64, device="cuda")
        _lib.check(lib.taoamd_bb_iou(d_dt.data_ptr(), d_gt.data_ptr(), m, n,
                                     None if d_col is None else d_col.data_ptr(),
                                     d_o.data_ptr(), None), "bb_iou")
        torch.cuda.synchronize()
        assert same_values(d_o.cpu().numpy().reshape((m, n), order="F"), ref_iou)
    if kind in ("scales", "far", "nonfinite"):
        assert not same_values(want, orclib.bb_iou(dt, gt, crowd))      # the column matters


# ---------------------------------------------------------------------------
# the fused match: every route
# ---------------------------------------------------------------------------
# test_gpu_match_routes.SIZE_CLASSES with further cells: the track level has
# one cell per entry, and the counts below ask for five cells of each class
BOX_SIZE_CLASSES = {
    "group": [8, 6, 8, 5, 7, 8, 3, 8, 4, 8, 2, 8],
    "single": [12, 40, 64, 9, 20, 33, 50, 16],
    "big": [65, 96, 97, 130, 66, 100, 80],
}
# seeds at which the ORACLE's tables hold what _nan_cells asks for (chosen on
# the host: see _match_flat)
MATCH_SEEDS = {("lvis", "group", "nonfinite"): 5, ("lvis", "single", "nonfinite"): 10}


@functools.lru_cache(maxsize=None)
def _rule_json(sizes):
    return fixtures.rule_cells(list(sizes), hidden_in=0)


def _match_flat(level, size_class, kind, seed=None):
    gtj, predj = _rule_json(tuple(BOX_SIZE_CLASSES[size_class]))
    gt, dt = GTColumns.from_json(gtj), DTColumns.from_json(predj)
    if seed is None:
        seed = MATCH_SEEDS.get((level, size_class, kind), 0)
    rng = np.random.default_rng([seed, KINDS.index(kind), len(size_class)])
    # (small cells want a larger share to hold two changed boxes at all)
    share = 0.35 if size_class == "group" else 0.12
    boxpop.implant(gt, dt, kind, rng, gt_share=share, dt_share=0.08)
    if level == "lvis":
        return fl.flatten_lvis(gt, dt)
    dt.track_id, _ = fl.make_track_ids_unique(dt)
    return fl.flatten_tao(gt, dt)


def _nan_cells(f, iou):
    """From the oracle's IoUs, per cell: (beside, closed, sequential) --
    `beside`: some detection has a NaN IoU and a finite IoU at or above the
    lowest threshold; `closed`: the cell holds a NaN IoU and no detection has
    two IoUs that pass ``!(v < lowest threshold)`` -- what the group kernel's
    closed form ("at most one candidate per detection: the greedy has no
    choice") would accept.  It must not: once a NaN is `best`, no later IoU is
    below it, so the reference hands the match to every later free ground
    truth in turn, candidate or not.  `sequential`: the cell holds a NaN IoU
    and some detection has two such IoUs or more, the group kernel's own test
    for its sequential loop.  Every cell that holds a NaN belongs in that
    loop; a cell without one and without a second candidate takes the closed
    form (`plain`)."""
    thr0 = orclib.thresholds()[0][0]
    off = orclib.iou_offsets(f)
    beside, closed = np.zeros(f.n_cells, bool), np.zeros(f.n_cells, bool)
    sequential, plain = np.zeros(f.n_cells, bool), np.zeros(f.n_cells, bool)
    for c in range(f.n_cells):
        D = f.cell_dt_off[c + 1] - f.cell_dt_off[c]
        G = f.cell_gt_off[c + 1] - f.cell_gt_off[c]
        if D and G:
            m = iou[off[c]:off[c + 1]].reshape(D, G)
            nan = np.isnan(m)
            with np.errstate(invalid="ignore"):
                cand = ~(m < thr0)
                beside[c] = (nan.any(axis=1) & (~nan & (m >= thr0)).any(axis=1)).any()
            multi = bool((cand.sum(axis=1) >= 2).any())
            closed[c] = nan.any() and not multi
            sequential[c] = nan.any() and multi
            plain[c] = not nan.any() and not multi
    return beside, closed, sequential, plain


def _check_nan_cells(size_class, f, iou, written=False):
    """At least 5 cells in which a detection has a NaN IoU beside a finite one
    at or above the lowest threshold.  In the group class, of the cells that
    hold a NaN, at least 2 look like closed-form cells but for it and at
    least 2 have a detection with two candidates (sequential on any count);
    and at least 2 cells without a NaN do take the closed form beside them
    (not asked of a table with NaNs `written` into nearly every cell)."""
    beside, closed, sequential, plain = _nan_cells(f, iou)
    counts = (beside.sum(), closed.sum(), sequential.sum(), plain.sum())
    assert beside.sum() >= 5, counts
    if size_class == "group":
        assert closed.sum() >= 2 and sequential.sum() >= 2, counts
        assert written or plain.sum() >= 2, counts


def _with_nan_entries(f, iou, seed):
    """The track level cannot produce a NaN IoU: a NaN term makes the union
    NaN, and ``u > 0 ? i / u : 0`` (per frame in avg_iou) answers 0; the
    imagenetvid IoU is a ratio of counts.  The match kernels that read their
    IoUs from a table are an entry point of their own, though
    (taoamd_match), so they get a table with NaNs written over a share of the
    oracle's IoUs -- beside the candidates, and alone in a cell."""
    rng = np.random.default_rng([seed, 77])
    out = iou.copy()
    off = orclib.iou_offsets(f)
    thr0 = orclib.thresholds()[0][0]
    for c in range(f.n_cells):
        G = int(f.cell_gt_off[c + 1] - f.cell_gt_off[c])
        m = out[off[c]:off[c + 1]].reshape(-1, G) if G else out[:0].reshape(0, 0)
        if m.size == 0:
            continue
        if c % 3 != 1:          # beside a candidate: in the rows that have one
            for d in np.flatnonzero((m >= thr0).any(axis=1)):
                free = np.flatnonzero(~(m[d] >= thr0))
                if len(free):
                    m[d, rng.choice(free)] = boxpop.NANS[rng.integers(0, 3)]
            m[rng.random(m.shape) < 0.03] = np.nan
        else:                   # alone: the cell keeps no other candidate
            m[m >= thr0] = 0.25
            m[rng.integers(0, m.shape[0]), rng.integers(0, G)] = np.nan
    return out


def _tao_match_on_table(f, iou, detail):
    """The track-level match and sweep on a given IoU table."""
    import torch
    from tao_amodal_amd import engine
    dp = engine.DeviceProblem(f)
    ws = engine.Workspace(dp, detail=detail, dt_rng_table=True)
    with _launches() as names:
        engine.stage_ranges(dp, ws)
        engine.stage_sort(dp, ws)
        ws.iou[:dp.n_iou] = torch.from_numpy(iou).to(dp.device)
        engine.stage_match(dp, ws)
        engine.stage_accumulate(dp, ws)
    torch.cuda.synchronize()
    n = dp.n_dt
    dst = ws.dst[:n].long()
    return dict(matched=ws.matched[:n][dst].cpu().numpy().view(np.uint64),
                ignored=ws.ignored[:n][dst].cpu().numpy().view(np.uint64),
                match_gt=ws.match_gt[:n].cpu().numpy() if detail else None,
                precision=ws.precision.cpu().numpy(), recall=ws.recall.cpu().numpy(),
                routes=names & MATCH_KERNELS)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("level", ["lvis", "tao"])
@pytest.mark.parametrize("size_class", list(BOX_SIZE_CLASSES))
def test_every_match_route_on_any_double(size_class, level, kind):
    """match_group_kernel (closed form and sequential), match_kernel and
    match_big_kernel, fused IoUs and IoUs from the table, with and without
    detail and in the production layout: a NaN IoU passes ``!(v < best)`` as it
    passes the reference's ``if iou < best: continue``, takes the match and
    hands it to whatever comes next.  Written as ``v >= best`` any of these
    kernels fails the nonfinite cases of its route."""
    import torch
    from tao_amodal_amd import engine
    f = _match_flat(level, size_class, kind)
    want = orclib.run_flat(f)
    if kind == "nonfinite" and level == "lvis":
        _check_nan_cells(size_class, f, want["iou"])
    elif kind in ("nonfinite", "scales"):
        # No NaN exists here.  Track level: see _with_nan_entries.  Image
        # level, `scales`: a detection survives on 0 < da < inf and the
        # intersection is at most da, so i is finite and u = da + ga - i is
        # +inf or a finite positive number (a negative w or h of a ground
        # truth, ga = -inf, leaves no intersection: 0 at once).  What the
        # population does give the match: IoUs that are exactly 0 through an
        # infinite union beside subnormal and ordinary ones.
        assert not np.isnan(want["iou"]).any()
        assert (want["iou"] == 0).any() and (want["iou"] > 0).any()
    dp = engine.DeviceProblem(f)
    want_routes = _routes(dp, f)
    assert {"group": "match_group_kernel", "single": "match_kernel",
            "big": "match_big_kernel"}[size_class] in want_routes
    for detail in (True, False):
        with _launches() as names:
            got = engine.evaluate_flat(f, detail=detail)
        assert names & MATCH_KERNELS == want_routes, (detail, names)
        _compare_with_oracle(f, got, detail=detail, equal_nan=True)
    if level != "lvis":
        if kind in ("nonfinite", "scales"):
            table = _with_nan_entries(f, want["iou"], KINDS.index(kind))
            _check_nan_cells(size_class, f, table, written=True)
            m, i, mg, _ = orclib.match(f, want["gt_rng"], want["dt_rng"], table)
            prec, rec, _, _ = orclib.accumulate(f, want["gt_rng"], m, i)
            for detail in (True, False):
                got = _tao_match_on_table(f, table, detail)
                assert got["routes"] == want_routes, got["routes"]
                assert np.array_equal(got["matched"], m)
                assert np.array_equal(got["ignored"], i)
                assert not detail or np.array_equal(got["match_gt"], mg)
                assert np.array_equal(got["precision"], prec)
                assert np.array_equal(got["recall"], rec)
        return
    ws = engine.Workspace(dp)
    with _launches() as names:
        engine.run(dp, ws)
    assert names & MATCH_KERNELS == want_routes, names
    torch.cuda.synchronize()
    n = dp.n_dt
    dst = ws.dst[:n].long()
    assert np.array_equal(ws.gt_rng[:dp.n_gt].cpu().numpy().view(np.uint32), want["gt_rng"])
    assert np.array_equal(ws.num_gt.cpu().numpy(), want["num_gt"])
    assert np.array_equal(ws.matched[:n][dst].cpu().numpy().view(np.uint64), want["matched"])
    assert np.array_equal(ws.ignored[:n][dst].cpu().numpy().view(np.uint64), want["ignored"])
    assert np.array_equal(ws.precision.cpu().numpy(), want["precision"])
    assert np.array_equal(ws.recall.cpu().numpy(), want["recall"])


# ---------------------------------------------------------------------------
# the three 3D-IoU kernels
# ---------------------------------------------------------------------------
TRACK_SETS = {
    "chunks": dict(seed=31, V=2, F=40, C=6, dets_per_frame=6, gt_tracks_per_video=4,
                   n_present=2, n_neg=1),
    "midchunk": dict(seed=32, V=1, F=37, C=6, dets_per_frame=8, gt_tracks_per_video=5,
                     n_present=2, n_neg=1),
}
ONE_FRAME = dict(seed=33, V=12, F=1, C=6, dets_per_frame=12, gt_tracks_per_video=6,
                 n_present=2, n_neg=1)


def _track_flat(kw, kind, holes):
    gt, dt = synth(**kw)
    if holes:
        gt, dt = _drop_frames(gt, dt, kw["seed"], keep=0.7)
    rng = np.random.default_rng([kw["seed"], KINDS.index(kind)])
    # (one NaN area makes a whole pair's union NaN and its IoU 0: few of them,
    # so that most pairs keep an IoU worth comparing)
    share = (0.04, 0.04) if kind == "nonfinite" and kw["F"] > 1 else (0.3, 0.15)
    boxpop.implant(gt, dt, kind, rng, gt_share=share[0], dt_share=share[1])
    dt.track_id, _ = fl.make_track_ids_unique(dt)
    return fl.flatten_tao(gt, dt)


def _far_counts(f):
    """(pairs with a real box beyond 1e300 in both axes -- x, y, x + w and
    y + h -- on a position the other track of the pair has no frame at, boxes
    at x == 1e300 exactly), from the tables."""
    def beyond(b):
        return (b[:, 0] > boxpop.FAR) & (b[:, 1] > boxpop.FAR) & \
            (b[:, 0] + b[:, 2] > boxpop.FAR) & (b[:, 1] + b[:, 3] > boxpop.FAR)
    db, gb = np.asarray(f.dt_frame_box), np.asarray(f.gt_frame_box)
    d_far, g_far = beyond(db), beyond(gb)
    pairs = 0
    for c in range(f.n_cells):
        for d in range(f.cell_dt_off[c], f.cell_dt_off[c + 1]):
            d0, d1 = f.dt_frame_off[d], f.dt_frame_off[d + 1]
            dpos = f.dt_frame_pos[d0:d1]
            for g in range(f.cell_gt_off[c], f.cell_gt_off[c + 1]):
                g0, g1 = f.gt_frame_off[g], f.gt_frame_off[g + 1]
                gpos = f.gt_frame_pos[g0:g1]
                alone = (d_far[d0:d1] & ~np.isin(dpos, gpos)).any() or \
                    (g_far[g0:g1] & ~np.isin(gpos, dpos)).any()
                pairs += bool(alone)
    return pairs, int((db[:, 0] == boxpop.FAR).sum() + (gb[:, 0] == boxpop.FAR).sum())


def _three_kernels(f, mode, single=False):
    """{kernel: (iou, pair_frames)} of the planned task kernel, the merge
    kernel and -- on a one-frame set -- taoamd_track_iou_single, each from a
    DeviceProblem of its own, with the kernel names that ran."""
    import torch
    from tao_amodal_amd import engine
    out = {}

    def run(dp):
        ws = engine.Workspace(dp)
        with _launches() as names:
            engine.stage_track_iou(dp, ws)
        torch.cuda.synchronize()
        return ws.iou[:dp.n_iou].cpu().numpy(), int(ws.pair_frames.item()), names
    if single:
        dp = engine.DeviceProblem(f, iou_3d_type=mode)
        assert dp.single_frame
        out["single"] = run(dp)
        assert "track_iou_single_kernel" in out["single"][2]
        os.environ["TAOAMD_SINGLE_FRAME"] = "0"
    try:
        dp = engine.DeviceProblem(f, iou_3d_type=mode)
    finally:
        os.environ.pop("TAOAMD_SINGLE_FRAME", None)
    assert not dp.single_frame
    out["planned"] = run(dp)
    out["has_plan"] = dp.t["tasks"] is not None
    dp.t["tasks"] = None
    out["merge"] = run(dp)
    assert out["merge"][2] & {"track_iou_kernel", "track_iou_task_kernel"} == {"track_iou_kernel"}
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", list(TRACK_SETS) + ["one_frame"])
def test_track_iou_kernels_on_any_double(which, kind):
    """The planned path, the merge kernel and the single-frame kernel in all
    three modes against the C oracle and each other, pair_frames included.
    The task kernel marks an absent frame with a box at x = y = 1e300: a table
    with a corner at or beyond that (or not finite) must not reach it -- a
    real box at x == 1e300 would be counted absent (pair_frames, avg_iou,
    imagenetvid).  Such tables take the merge kernel; all others must still
    take the task kernel."""
    single = which == "one_frame"
    f = _track_flat(ONE_FRAME if single else TRACK_SETS[which], kind, holes=not single)
    if kind == "far":
        pairs, at_far = _far_counts(f)
        assert at_far >= 3, at_far
        if not single:          # (a one-frame pair that shares no frame has IoU 0 by any arithmetic)
            assert pairs >= 10, pairs
    n_common = None
    for mode in MODES:
        want, want_pairs = orclib.track_iou(f, mode)
        got = _three_kernels(f, mode, single)
        for k in ("planned", "merge") + (("single",) if single else ()):
            iou, pf, _ = got[k]
            assert same_values(iou, want), (k, mode)
            assert pf == want_pairs, (k, mode, pf, want_pairs)
        # (the values first: what a kernel that met its own sentinel gets wrong)
        in_domain = kind not in ("far", "nonfinite")
        assert got["has_plan"] == in_domain
        assert ("track_iou_task_kernel" in got["planned"][2]) == in_domain, got["planned"][2]
        assert n_common in (None, want_pairs)
        n_common = want_pairs
    assert n_common > 0


def test_task_kernel_still_runs_every_ordinary_table():
    """The domain test of taoamd_track_pad must not send ordinary tables --
    integer, decimal, negative, 1e150 -- to the slow kernel, and a single
    coordinate at 1e300, above it, or NaN must."""
    import torch
    from tao_amodal_amd import engine
    f = _track_flat(TRACK_SETS["chunks"], "amodal", holes=True)
    assert engine.DeviceProblem(f).t["tasks"] is not None
    row = int(np.flatnonzero(np.diff(f.gt_frame_off) > 2)[0])
    k = int(f.gt_frame_off[row]) + 1
    for col, v, planned in ((0, 9.9e299, True), (0, -9.9e299, True), (0, 1e300, False),
                            (1, -1e300, False), (0, np.nextafter(1e300, np.inf), False),
                            (2, 1e300, False), (3, np.nan, False), (1, np.inf, False),
                            (0, np.nextafter(1e300, 0), True)):
        g = copy.copy(f)
        box = np.array(f.gt_frame_box)
        box[k, col] = v
        g.gt_frame_box = box
        dp = engine.DeviceProblem(g)
        assert (dp.t["tasks"] is not None) == planned, (col, v)
        ws = engine.Workspace(dp)
        engine.stage_track_iou(dp, ws)
        torch.cuda.synchronize()
        want, pairs = orclib.track_iou(g)
        assert same_values(ws.iou[:dp.n_iou].cpu().numpy(), want), (col, v)
        assert int(ws.pair_frames.item()) == pairs


# ---------------------------------------------------------------------------
# identical decimal tracks through the class API
# ---------------------------------------------------------------------------
def test_predictions_copied_from_a_decimal_ground_truth():
    """The reference's ``assert i <= u`` fires on a box against its own copy
    ((x + w) - x > w by rounding: about a third of decimal boxes); the product
    returns i / u, just above 1, and goes on.  Through TaoEval and LVISEval:
    the run completes and equals the C oracle, AP included."""
    from tao_amodal_amd.evaluation.lvis_amodal import LVIS, LVISEval, LVISResults
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval, TaoResults
    gt, _ = synth(seed=34, V=3, F=12, C=6, dets_per_frame=4, gt_tracks_per_video=5,
                  n_present=2, n_neg=1, decimal=True)
    n = len(gt.ann_id)
    vid_of_img = dict(zip(gt.img_id.tolist(), gt.img_vid.tolist()))
    dt = DTColumns(image_id=gt.ann_img.copy(), category_id=gt.ann_cat.copy(),
                   bbox=gt.ann_bbox.copy(),
                   score=np.random.default_rng(34).random(n).round(3),
                   track_id=gt.ann_trk.copy(),
                   video_id=np.array([vid_of_img[i] for i in gt.ann_img.tolist()], np.int64))
    gtj = gt.to_json()
    f = fl.flatten_tao(gt, dt)
    want = orclib.run_flat(f, detail=False)
    assert (want["iou"] > 1).sum() > 0                   # (the oracle's)
    lf = fl.flatten_lvis(gt, dt)
    lwant = orclib.run_flat(lf)
    assert (lwant["iou"] > 1).sum() > 0
    g = Tao(gtj)
    te = TaoEval(g, TaoResults(g, dt))
    te.run()
    assert np.array_equal(te.eval["precision"].reshape(want["precision"].shape),
                          want["precision"])
    assert np.array_equal(te.eval["recall"].reshape(want["recall"].shape), want["recall"])
    p = want["precision"][:, :, :, 0]
    assert te.results["AP"] == np.mean(p[p > -1])
    g = LVIS(gtj)
    le = LVISEval(g, LVISResults(g, dt), "bbox")
    le.run()
    assert np.array_equal(le.eval["precision"], lwant["precision"])
    assert np.array_equal(le.eval["recall"], lwant["recall"])
    p = lwant["precision"][:, :, :, 0]
    assert le.results["AP"] == np.mean(p[p > -1])
    assert le.results["AP"] > 0.9 and te.results["AP"] > 0.9


# ---------------------------------------------------------------------------
# the device table build
# ---------------------------------------------------------------------------
TABLE_SET = dict(seed=35, V=3, F=10, C=12, dets_per_frame=20, n_present=4)


def _table_inputs(kind):
    gt, dt = synth(**TABLE_SET)
    rng = np.random.default_rng([35, KINDS.index(kind)])
    g_rows, d_rows = boxpop.implant(gt, dt, kind, rng, gt_share=0.3, dt_share=0.3)
    return gt, dt, d_rows


@pytest.mark.parametrize("kind", KINDS)
def test_lvis_device_tables_on_any_double(kind):
    """flatten_lvis_device against flatten.py: the rows kept by 0 < w * h <
    inf (NaN, infinite, negative, underflowed and overflowed areas on either
    side of it), their order, and the flag of the 1e5 ** 2 bound."""
    from test_gpu_flatten import LVIS_FIELDS, _same
    from tao_amodal_amd import flatten_dev
    gt, dt, d_rows = _table_inputs(kind)
    want = fl.flatten_lvis(gt, dt)
    kept = np.isin(d_rows, want.dt_row)
    if kind in ("scales", "nonfinite", "far"):
        assert kept.any() and not kept.all()            # the filter has work on both sides
    _same(flatten_dev.flatten_lvis_device(gt, dt, "cuda:0"), want, LVIS_FIELDS)
    if kind in ("scales", "far"):                        # the area bound on the device
        a = want.dt_box[:, 2] * want.dt_box[:, 3]
        assert (a > 1e10).any() and (a < 1e10).any()


@pytest.mark.parametrize("kind", KINDS)
def test_tao_device_tables_on_any_double(kind):
    """flatten_tao_device against flatten.py: kept rows, order, dt_area (the
    track's mean area), the area-range flags."""
    from test_gpu_flatten import TAO_FIELDS, _same
    from tao_amodal_amd import flatten_dev
    gt, dt, _ = _table_inputs(kind)
    dt.track_id, _ = fl.make_track_ids_unique(dt)
    want = fl.flatten_tao(gt, dt)
    got = flatten_dev.flatten_tao_device(gt, dt, "cuda:0")
    _same(got, want, TAO_FIELDS)
    assert got.required_average == want.required_average


# ---------------------------------------------------------------------------
# the device JSON reader
# ---------------------------------------------------------------------------
def _spell(v):
    if v != v:
        return "NaN"
    if v in (np.inf, -np.inf):
        return "Infinity" if v > 0 else "-Infinity"
    return repr(float(v))


@pytest.mark.parametrize("kind", KINDS)
def test_device_json_reader_on_any_double(kind, tmp_path, monkeypatch):
    """A prediction file with repr-exact decimals (exponents to e+308, 5e-324)
    and the NaN / Infinity literals: the device reader's columns are the host
    reader's, as bits, or it steps aside for the host reader."""
    import torch  # noqa: F401
    from test_gpu_ingest import device, host, same
    monkeypatch.setattr(DTColumns, "DEVICE_INGEST_MIN_BYTES", 0)
    rng = np.random.default_rng([36, KINDS.index(kind)])
    box = boxpop.box_population(kind, 4000, rng)
    objs = ['{"image_id": %d, "category_id": %d, "bbox": [%s], "score": %s, "track_id": %d, '
            '"video_id": 1}' % (k + 1, k % 7 + 1, ", ".join(_spell(v) for v in b),
                                repr(float(rng.random())), k)
            for k, b in enumerate(box)]
    p = str(tmp_path / "pred.json")
    with open(p, "w") as fh:
        fh.write("[" + ",\n".join(objs) + "]\n")
    want = host(p)
    # the host reader itself: every value back as written (NaN as a NaN)
    assert same_values(want.bbox, box)
    if kind != "nonfinite":
        assert np.array_equal(want.bbox.view(np.uint64), box.view(np.uint64))
        assert [json.loads(o)["bbox"] for o in objs[:50]] == box[:50].tolist()
    got = device(p)
    if got is not None:
        same(got, want)
    same(DTColumns.from_file_native(p), want)


# ---------------------------------------------------------------------------
# taoamd_error_types
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_error_types_on_any_double(kind):
    """Against tests/error_types_ref.py.  A NaN overlap is no overlap (the
    header's definition): left out of s, o and the argmax."""
    from test_gpu_error_types import _device_error_types, _device_match, _same
    f = _match_flat("lvis", "single", kind, seed=3)
    gt_rng, _ = orclib.ranges(f)
    thrs, _ = orclib.thresholds()
    if kind == "nonfinite":
        d_img, g_img = ref.units(f)
        n_nan = sum(int(np.isnan(orclib.bb_iou(f.dt_box[d_img == u], f.gt_box[g_img == u])).sum())
                    for u in np.unique(d_img))
        assert n_nan >= 20, n_nan
    mg = _device_match(f, gt_rng, 6)
    assert np.array_equal(mg, orclib.run_flat(f)["match_gt"])
    for slot, tb in ((0, 0.1), (5, 0.25)):
        want = ref.error_types(f, mg, gt_rng, thrs, slot, tb)
        assert len(np.unique(want["dt_type"])) >= 3
        _same(_device_error_types(f, mg, gt_rng, 6, slot, tb), want)
