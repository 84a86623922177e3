"""-m gpu: the track-level error breakdown (taoamd_track_error_types,
engine.stage_track_error_types, TaoEval.error_types) against the numpy
restatement of tests/track_error_types_ref.py.  The restatement's IoUs are the C
oracle's, the kernels' arithmetic in the kernels' order: every comparison is
exact."""
import sys

import numpy as np
import pytest

import boxpop
import error_types_ref as img_ref
import orclib
import track_error_types_ref as ref
import wsguard
from goldenio import GOLDEN as GOLDEN_DIR, input_paths, path
from tao_amodal_amd import _lib

sys.path.insert(0, GOLDEN_DIR)
from constants_cases import cases, edit  # noqa: E402

pytestmark = pytest.mark.gpu

N_THR = _lib.N_THR
TILE = _lib.TRACK_ERROR_TYPES_TILE
DEV = "cuda:0"


def _up(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], dtype=dtype)
    return torch.from_numpy(a).to(DEV)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _frames(t):
    """The six frame-list columns of a track table on the device."""
    return [_up(t.dt_frame_off, np.int32), _up(t.dt_frame_pos, np.int32),
            _up(np.asarray(t.dt_frame_box, dtype=np.float64).reshape(-1, 4), np.float64),
            _up(t.gt_frame_off, np.int32), _up(t.gt_frame_pos, np.int32),
            _up(np.asarray(t.gt_frame_box, dtype=np.float64).reshape(-1, 4), np.float64)]


def _device_match(f, iou, gt_rng, dt_rng, n_rng):
    """match_gt[n_dt, n_rng * 10] of taoamd_match itself (one wavefront per cell)
    on the oracle's IoU matrix."""
    import torch
    lib = _lib.load()
    n_dt = int(f.cell_dt_off[-1])
    nw = (n_rng * N_THR + 63) // 64
    cols = [_up(f.cell_dt_off, np.int32), _up(f.cell_gt_off, np.int32),
            _up(f.cell_iou_off, np.int64), _up(iou, np.float64),
            _up(gt_rng, np.uint32).view(torch.int32), _up(dt_rng, np.uint32).view(torch.int32),
            _up(f.gt_flags, np.uint8), _up(f.dt_flags, np.uint8)]
    d_off, g_off, i_off, iou_t, grng, drng, gfl, dfl = [c.data_ptr() for c in cols]
    matched = torch.zeros((max(n_dt, 1), nw), dtype=torch.int64, device=DEV)
    ignored = torch.zeros_like(matched)
    mg = torch.full((max(n_dt, 1), n_rng * N_THR), -7, dtype=torch.int32, device=DEV)
    max_g = int(np.diff(f.cell_gt_off).max()) if f.n_cells else 0
    _lib.check(lib.taoamd_match(
        f.n_cells, d_off, g_off, i_off, max_g, None, None, iou_t, n_rng, grng, drng, gfl, dfl,
        None, 0, matched.data_ptr(), ignored.data_ptr(), mg.data_ptr(), None, None, None,
        None, 0, None, 0, _stream()), "taoamd_match")
    torch.cuda.synchronize()
    return mg[:n_dt].cpu().numpy()


def _device_pooled_iou(f):
    """The plan-less taoamd_track_iou on the cells pooled per video: every
    (detection track, ground-truth track) pair of a video."""
    import torch
    lib = _lib.load()
    t, _, _ = ref.pooled(f)
    n = int(t.cell_iou_off[-1])
    out = torch.full((max(n, 1),), -5.0, dtype=torch.float64, device=DEV)
    cols = [_up(t.cell_dt_off, np.int32), _up(t.cell_gt_off, np.int32),
            _up(t.cell_iou_off, np.int64)] + _frames(t)
    if n:
        _lib.check(lib.taoamd_track_iou(
            t.n_cells, *[c.data_ptr() for c in cols[:3]], n, *[c.data_ptr() for c in cols[3:]],
            0, out.data_ptr(), None, _stream()), "taoamd_track_iou")
    torch.cuda.synchronize()
    return out[:n].cpu().numpy()


def _csr(unit, n_unit, rows=None):
    off = np.zeros(n_unit + 1, np.int32)
    np.cumsum(np.bincount(unit, minlength=n_unit), out=off[1:])
    rows = np.argsort(unit, kind="stable") if rows is None else rows
    return off, rows


def _device_error_types(f, iou, mg, gt_rng, dt_rng, n_rng, slot, tb, per_detection=True,
                        over=True, status=False, ws_bytes=None, lists=None):
    """taoamd_track_error_types on a Flat; the workspace is exactly the size
    reported, behind a guard band.  `lists`: (vid_gt_off, vid_gt, vid_dt_off,
    vid_dt) instead of the table's own."""
    import torch
    lib = _lib.load()
    n_dt, n_gt = int(f.cell_dt_off[-1]), int(f.cell_gt_off[-1])
    n_vid, K = len(f.vid_ids), len(f.cat_ids)
    d_vid, g_vid = ref.units(f)
    if lists is None:
        lists = _csr(g_vid, n_vid) + _csr(d_vid, n_vid)
    lists = [_up(x, np.int32) for x in lists]
    d_off, g_off = np.asarray(f.cell_dt_off), np.asarray(f.cell_gt_off)
    d_cell = np.repeat(np.arange(f.n_cells), np.diff(d_off))
    group = np.stack([g_off[d_cell], np.diff(g_off)[d_cell], np.arange(n_dt) - d_off[d_cell],
                      d_cell], 1) if n_dt else np.zeros((0, 4))
    cols = [_up(f.dt_cat, np.int32), _up(dt_rng, np.uint32).view(torch.int32),
            _up(group, np.int32), _up(f.cell_iou_off, np.int64), _up(iou, np.float64),
            _up(mg, np.int32)]
    gcols = [_up(f.gt_cat, np.int32), _up(gt_rng, np.uint32).view(torch.int32)]
    fr = _frames(f)
    dt_counts = torch.full((n_rng, K, 7), -3, dtype=torch.int64, device=DEV)
    gt_counts = torch.full((n_rng, K, 3), -3, dtype=torch.int64, device=DEV)
    dt_type = torch.full((max(n_dt, 1), n_rng), 99, dtype=torch.uint8, device=DEV)
    dt_over = torch.full((max(n_dt, 1), 2), -1, dtype=torch.int32, device=DEV)
    need = lib.taoamd_track_error_types_workspace(n_dt, n_gt, min(max(n_rng, 1), 20))
    ws = wsguard.Guarded(need if ws_bytes is None else ws_bytes, DEV)
    st = lib.taoamd_track_error_types(
        n_dt, n_gt, f.n_cells, len(iou), n_vid, K, n_rng, slot, tb,
        *[c.data_ptr() for c in cols], np.asarray(mg).reshape(max(n_dt, 1), -1).shape[1],
        *[c.data_ptr() for c in gcols], *[c.data_ptr() for c in fr],
        *[c.data_ptr() for c in lists], dt_counts.data_ptr(), gt_counts.data_ptr(),
        dt_type.data_ptr() if per_detection else None, dt_over.data_ptr() if over else None,
        ws.data_ptr(), ws.nbytes, _stream())
    if status:
        torch.cuda.synchronize()
        return st
    _lib.check(st, "taoamd_track_error_types")
    ws.check()
    return dict(dt_counts=dt_counts.cpu().numpy(), gt_counts=gt_counts.cpu().numpy(),
                dt_type=dt_type[:n_dt].cpu().numpy() if per_detection else None,
                dt_over=dt_over[:n_dt].cpu().numpy().view(np.uint32) if over else None)


def _same(got, want):
    assert np.array_equal(got["dt_counts"], want["dt_counts"])
    assert np.array_equal(got["gt_counts"], want["gt_counts"])
    if got["dt_type"] is not None:
        assert np.array_equal(got["dt_type"], want["dt_type"])
    if got["dt_over"] is not None:
        assert np.array_equal(got["dt_over"], want["dt_over"])


def test_abi_on_the_hand_written_table():
    f, dt_at, gt_at = ref.hand_flat()
    gt_rng, dt_rng = orclib.ranges(f)
    iou, _ = orclib.track_iou(f)
    thrs, _ = orclib.thresholds()
    mg = _device_match(f, iou, gt_rng, dt_rng, 20)
    got = _device_error_types(f, iou, mg, gt_rng, dt_rng, 20, 0, ref.HAND_TB)
    assert got["dt_type"][dt_at, 0].tolist() == ref.HAND_TYPES_RNG0
    assert got["dt_type"][dt_at, 1].tolist() == ref.HAND_TYPES_RNG1
    assert got["dt_type"][dt_at, 3].tolist() == ref.HAND_TYPES_RNG3
    assert got["dt_counts"][0].tolist() == ref.HAND_DT_COUNTS_RNG0
    assert got["gt_counts"][0].tolist() == ref.HAND_GT_COUNTS_RNG0
    assert got["gt_counts"][3].tolist() == ref.HAND_GT_COUNTS_RNG3
    for d in range(len(ref.HAND_DETS)):
        want = ref.HAND_OVER_RNG0.get(d, (0, 0))
        assert tuple(int(w) & 1 for w in got["dt_over"][dt_at[d]]) == want, d
    _same(got, ref.error_types(f, iou, mg, gt_rng, dt_rng, thrs, 0, ref.HAND_TB))
    # just above tb the rows pinned at exactly tb fall to BKG
    up = _device_error_types(f, iou, mg, gt_rng, dt_rng, 20, 0, 0.125 + 2.0 ** -50)
    assert up["dt_type"][dt_at[[9, 11]], 0].tolist() == [ref.BKG, ref.BKG]
    _same(up, ref.error_types(f, iou, mg, gt_rng, dt_rng, thrs, 0, 0.125 + 2.0 ** -50))
    # another slot: tf = 0.75; and no background threshold at all
    _same(_device_error_types(f, iou, mg, gt_rng, dt_rng, 20, 5, 0.3),
          ref.error_types(f, iou, mg, gt_rng, dt_rng, thrs, 5, 0.3))
    _same(_device_error_types(f, iou, mg, gt_rng, dt_rng, 20, 0, 0.0),
          ref.error_types(f, iou, mg, gt_rng, dt_rng, thrs, 0, 0.0))


# (ground-truth tracks, detection tracks) per video: every pairing of the sizes
# around the kernel's tile of ground-truth tracks and around a wavefront / a
# workgroup's lanes; then a video whose ground truths all share one category
GTS = sorted({0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1})
DTS = [0, 1, 63, 64, 65, 257]
VIDEOS = [(g, d) for g in GTS for d in DTS] + [(TILE, 64)]
ONE_CAT_VIDEO = len(VIDEOS) - 1
N_CAT = 4
LENGTHS = [1, 7, 8, 9, 64, 65]


def _seeded_table(seed, boxes=None):
    """Tracks of LENGTHS frames with gaps on a timeline of 130 positions (spans
    that do not meet; tracks in the last third share no frame with any ground
    truth placed in the first two).  Integer boxes that move by a pixel, or
    `boxes(n)`: n pairs (detection's side, ground truth's side) of any double."""
    rng = np.random.default_rng(seed)

    def positions():
        n = int(rng.choice(LENGTHS))
        span = min(130, n + int(rng.integers(0, n + 1)))
        lo = int(rng.integers(0, 130 - span + 1))
        return np.sort(lo + rng.choice(span, n, replace=False))

    def still(pos, box):
        if boxes is not None:
            return None
        x, y, w, h = box
        return {int(p): [x + int(rng.integers(0, 2)), y, w, h] for p in pos}

    def box():
        x, y = rng.integers(0, 6, 2) * 4
        w, h = rng.choice([4, 8, 16], 2)
        return [int(x), int(y), int(w), int(h)]
    dets, gts = [], []
    for v, (ng, nd) in enumerate(VIDEOS):
        mine = []
        for _ in range(ng):
            pos = positions()
            pos = pos[pos < 87] if (pos < 87).any() else pos % 87
            pos = np.unique(pos)
            cat = 0 if v == ONE_CAT_VIDEO else int(rng.integers(N_CAT))
            bx = box()
            fr = still(pos, bx)
            if boxes is not None:
                pop = boxes(len(pos))
                fr = {int(p): pop[2 * k + 1].tolist() for k, p in enumerate(pos)}
                mine.append((cat, pos, pop))
            else:
                mine.append((cat, pos, bx))
            gts.append((v, cat, fr, int(rng.choice([0, 0, 0, 0, 1])),
                        float(rng.choice([100.0, 2000.0, 20000.0])), int(rng.choice([0, 10]))))
        for _ in range(nd):
            cat, pos, bx = int(rng.integers(N_CAT)), positions(), box()
            r = rng.random()
            if r < 0.15:
                pos = np.unique(87 + pos % 43)       # shares no frame with a ground truth
            pop = None
            if ng and r >= 0.5:                      # on a ground truth: TPs, DUPs, CLS
                gcat, gpos, gbx = mine[int(rng.integers(ng))]
                keep = rng.random(len(gpos)) < rng.choice([0.5, 0.8, 1.0])
                pos = gpos[keep] if keep.any() else gpos
                cat = gcat if rng.random() < 0.5 else cat
                if boxes is None:
                    bx = gbx
                else:
                    pop = gbx[np.repeat(keep if keep.any() else np.ones(len(gpos), bool), 2)]
            if boxes is None:
                fr = still(pos, bx)
            else:
                pop = boxes(len(pos)) if pop is None else pop
                fr = {int(p): pop[2 * k].tolist() for k, p in enumerate(pos)}
            dets.append((v, cat, fr, float(rng.integers(0, 50)) / 50,
                         int(rng.choice([0, 0, 0, 1, 2])),
                         float(rng.choice([100.0, 2000.0, 20000.0]))))
    f, _, _ = ref.make_track_flat(len(VIDEOS), N_CAT, dets, gts)
    return f


@pytest.fixture(scope="module")
def seeded_tables():
    """{n_rng: (flat, iou, gt_rng, dt_rng, match_gt of taoamd_match, restatement
    at (slot 0, tb 0.1) and (slot 5, tb 0.25))}."""
    out = {}
    thrs, _ = orclib.thresholds()
    for n_rng in (1, 20):
        f = _seeded_table(50 + n_rng)
        gt_rng, dt_rng = orclib.ranges(f)
        iou, _ = orclib.track_iou(f)
        mg = _device_match(f, iou, gt_rng, dt_rng, n_rng)
        want = {(t, tb): ref.error_types(f, iou, mg, gt_rng, dt_rng, thrs, t, tb, n_rng)
                for t, tb in ((0, 0.1), (5, 0.25))}
        for w in want.values():
            for v in w.values():
                v.setflags(write=False)
        out[n_rng] = (f, iou, gt_rng, dt_rng, mg, want)
    return out


@pytest.mark.parametrize("slot,tb", [(0, 0.1), (5, 0.25)])
@pytest.mark.parametrize("n_rng", [1, 20])
def test_abi_on_seeded_tables(seeded_tables, n_rng, slot, tb):
    f, iou, gt_rng, dt_rng, mg, want = seeded_tables[n_rng]
    w = want[slot, tb]
    # the cases are there: every type, long and short tracks, most pairs cross-category
    assert set(np.unique(w["dt_type"])) == set(range(7))
    assert (mg >= 0).any() and (mg == -1).any() and (mg >= -1).all()
    lens = np.diff(f.dt_frame_off)
    assert set(ref_len for ref_len in LENGTHS if (lens == ref_len).any()) == set(LENGTHS)
    assert int(f.dt_frame_pos.max()) >= 120
    assert w["gt_counts"][..., 2].any() and (w["o"] >= 0.5).any()
    tf = img_ref.foreground(orclib.thresholds()[0], slot)
    assert ((w["o"] >= tb) & (w["o"] < tf)).any()
    got = _device_error_types(f, iou, mg, gt_rng, dt_rng, n_rng, slot, tb)
    _same(got, w)
    # device against device: the pairs' IoUs of the plan-less kernel on the
    # video-pooled cells give the same masks -- the new kernel adds in its order
    pooled_iou = _device_pooled_iou(f)
    over, _ = ref.over_masks(f, ref.cross_blocks(f, iou=pooled_iou), gt_rng, tf, tb, n_rng)
    assert np.array_equal(got["dt_over"], over)
    assert np.array_equal(pooled_iou, orclib.track_iou(ref.pooled(f)[0])[0], equal_nan=True)
    # the video whose ground truths all share one category: no cross-category overlap
    d_vid, _ = ref.units(f)
    one = (d_vid == ONE_CAT_VIDEO) & (np.asarray(f.dt_cat) == 0)
    assert one.any() and not got["dt_over"][one].any()
    # the stated consequence: an unmatched row with s >= tf points at a held ground truth
    for a in range(n_rng):
        dup = np.flatnonzero(w["dt_type"][:, a] == ref.DUP)
        assert w["hit"][a, w["arg"][dup, a]].all()


def test_abi_on_boxes_that_are_any_double():
    """Coordinates from every population of tests/boxpop.py (NaN, +-inf, 1e300,
    negative w and h): dt_over and the types equal the restatement's, a NaN IoU
    is no overlap."""
    prng = np.random.default_rng(77)
    turn = [0]

    def boxes(n):
        kind = boxpop.KINDS[turn[0] % len(boxpop.KINDS)]
        turn[0] += 1
        return boxpop.box_population(kind, 2 * n, prng)
    f = _seeded_table(91, boxes)
    gt_rng, dt_rng = orclib.ranges(f)
    with np.errstate(all="ignore"):
        iou, _ = orclib.track_iou(f)
        cross = np.concatenate([m.ravel() for _, _, m in ref.cross_blocks(f)])
    assert np.isnan(cross).any() and np.isnan(iou).any() and (cross > 0.5).any()
    thrs, _ = orclib.thresholds()
    mg = _device_match(f, iou, gt_rng, dt_rng, 20)
    for slot, tb in ((0, 0.1), (5, 0.0)):
        with np.errstate(all="ignore"):
            want = ref.error_types(f, iou, mg, gt_rng, dt_rng, thrs, slot, tb)
        _same(_device_error_types(f, iou, mg, gt_rng, dt_rng, 20, slot, tb), want)


def test_abi_counts_do_not_depend_on_the_optional_outputs(seeded_tables):
    f, iou, gt_rng, dt_rng, mg, want = seeded_tables[20]
    for per, over in ((False, False), (True, False), (False, True)):
        got = _device_error_types(f, iou, mg, gt_rng, dt_rng, 20, 0, 0.1, per_detection=per,
                                  over=over)
        assert (got["dt_type"] is None) == (not per) and (got["dt_over"] is None) == (not over)
        _same(got, want[0, 0.1])


def test_abi_with_the_workspace_base_moved_by_8_bytes(seeded_tables, monkeypatch):
    monkeypatch.setattr(wsguard, "SHIFT", 8)
    f, iou, gt_rng, dt_rng, mg, want = seeded_tables[20]
    _same(_device_error_types(f, iou, mg, gt_rng, dt_rng, 20, 5, 0.25), want[5, 0.25])


def test_abi_error_paths(seeded_tables):
    f, iou, gt_rng, dt_rng, mg, want = seeded_tables[1]
    lib = _lib.load()
    call = lambda **kw: _device_error_types(                                # noqa: E731
        f, iou, mg, gt_rng, dt_rng, kw.pop("n_rng", 1), kw.pop("slot", 0), kw.pop("tb", 0.1),
        status=True, **kw)
    assert call(slot=10) == 2 and call(slot=-1) == 2
    assert call(tb=0.5) == 2 and call(tb=0.9) == 2 and call(tb=-0.1) == 2
    assert call(n_rng=21) == 2 and call(n_rng=0) == 2
    need = lib.taoamd_track_error_types_workspace(int(f.cell_dt_off[-1]),
                                                  int(f.cell_gt_off[-1]), 1)
    assert call(ws_bytes=need - 1) == 4
    assert call() == 0


def test_abi_rows_outside_the_tables_are_skipped(seeded_tables):
    """Row lists and match indices that name rows outside the tables: such a
    ground truth is in no video's set, such a detection row is listed nowhere,
    such a match is none.  The kernels bound-check; nothing is dereferenced."""
    f, iou, gt_rng, dt_rng, mg, _ = seeded_tables[20]
    n_dt, n_gt, n_vid = int(f.cell_dt_off[-1]), int(f.cell_gt_off[-1]), len(f.vid_ids)
    thrs, _ = orclib.thresholds()
    rng = np.random.default_rng(5)
    d_vid, g_vid = ref.units(f)
    g_off, g_rows = _csr(g_vid, n_vid)
    d_off, d_rows = _csr(d_vid, n_vid)
    g_bad = rng.choice(n_gt, 25, replace=False)
    d_bad = rng.choice(n_dt, 60, replace=False)
    junk = np.array([n_gt, n_gt + 7, 2 ** 31 - 1, -1, -2 ** 31])
    g_rows, d_rows = g_rows.copy(), d_rows.copy()
    g_rows[np.isin(g_rows, g_bad)] = junk[np.arange(25) % 5]
    d_rows[np.isin(d_rows, d_bad)] = (junk + n_dt - n_gt)[np.arange(60) % 5]
    mg2 = mg.copy()
    m_bad = rng.random(mg.shape) < 0.02
    mg2[m_bad] = rng.choice([10 ** 6, 2 ** 31 - 1, -5, -2 ** 31], int(m_bad.sum()))
    gl, dl = np.ones(n_gt, bool), np.ones(n_dt, bool)
    gl[g_bad], dl[d_bad] = False, False
    want = ref.error_types(f, iou, mg2, gt_rng, dt_rng, thrs, 0, 0.1, dt_listed=dl, gt_listed=gl)
    got = _device_error_types(f, iou, mg2, gt_rng, dt_rng, 20, 0, 0.1,
                              lists=(g_off, g_rows, d_off, d_rows))
    _same(got, want)
    assert not got["dt_over"][d_bad].any()


# ---------------------------------------------------------------------------
# the class API
# ---------------------------------------------------------------------------
def _tao(name, tmp_path=None, **kw):
    from tao_amodal_amd import flatten
    from tao_amodal_amd.columns import DTColumns
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval, TaoResults
    if tmp_path is None:
        gt_path, dt_path = path(name, "gt.json"), path(name, "pred.json")
    else:
        gt_path, dt_path = input_paths(name, tmp_path)
    dt = DTColumns.from_json(dt_path)
    dt.track_id, _ = flatten.make_track_ids_unique(dt)
    gt = Tao(gt_path)
    return TaoEval(gt, TaoResults(gt, dt), **kw)


def _restated(ev, iou_thr, bg_thr):
    """The restatement on the evaluator's own tables: IoU matrix, match indices
    and range masks of a detail-mode pass under the evaluator's constants, the
    kernel's range slots put in the caller's order."""
    import torch
    from tao_amodal_amd import engine
    from tao_amodal_amd.evaluation._core import applied
    run = ev._run
    c = run.constants
    ws = engine.Workspace(run.dp, detail=True)
    with applied(c):
        engine.run_guarded(run.dp, ws, run.flat, upto="match")
        torch.cuda.synchronize()
    n_dt, n_gt = run.dp.n_dt, run.dp.n_gt
    mg = ws.match_gt[:n_dt].cpu().numpy()
    gt_rng = ws.gt_rng[:n_gt].cpu().numpy().view(np.uint32)
    dt_rng = ws.dt_rng[:n_dt].cpu().numpy().view(np.uint32)
    iou = ws.iou[:run.dp.n_iou].cpu().numpy()
    thrs = orclib.thresholds()[0] if c is None else c.thr_blocks[0][1]
    i = int(np.where(iou_thr == np.asarray(ev.params.iou_thrs))[0][0])
    slot = i if c is None else int(np.where(c.thr_blocks[0][0] == i)[0][0])
    assert thrs[slot] == iou_thr
    want = ref.error_types(run.flat, iou, mg, gt_rng, dt_rng, thrs, slot, bg_thr)
    want = {k: want[k] for k in ("dt_counts", "gt_counts", "dt_type")}
    A, T = len(ev.params.area_rng), len(ev.params.time_rng)
    if (A, T) != (5, 4):
        # the kernels' slots of the caller's ranges: its areas from slot 0 on,
        # its last area in the occlusion slot 4; its durations from slot 0 on
        ks = [(a if a < A - 1 else 4) * 4 + t for a in range(A) for t in range(T)]
        want = dict(dt_counts=want["dt_counts"][ks], gt_counts=want["gt_counts"][ks],
                    dt_type=want["dt_type"][:, ks])
    cats = np.asarray(run.flat.cat_ids).tolist()
    pos = [cats.index(int(c)) for c in ev.params.cat_ids]
    want["dt_counts"], want["gt_counts"] = want["dt_counts"][:, pos], want["gt_counts"][:, pos]
    return want


def _check_class_api(ev, iou_thr, bg_thr):
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.error_types(iou_thr, bg_thr)
    ev.evaluate()
    want = _restated(ev, iou_thr, bg_thr)
    got = ev.error_types(iou_thr, bg_thr)
    assert "dt_type" not in got and got["types"] == list(ref.TYPES)
    P = ev.params
    n_rng, K = len(P.area_rng) * len(P.time_rng), len(P.cat_ids)
    assert len(got["rng_lbl"]) == n_rng and got["rng_lbl"][0] == ("all", "all")
    assert got["rng_lbl"][1] == (P.area_rng_lbl[0], P.time_rng_lbl[1])
    assert got["dt_counts"].shape == (n_rng, K, 7) and got["dt_counts"].dtype == np.int64
    assert got["gt_counts"].shape == (n_rng, K, 3)
    assert np.array_equal(got["dt_counts"], want["dt_counts"])
    assert np.array_equal(got["gt_counts"], want["gt_counts"])
    assert ev.error_types(iou_thr, bg_thr)["dt_counts"] is got["dt_counts"]     # cached
    per = ev.error_types(iou_thr, bg_thr, per_detection=True)
    ids, types = per["dt_type"]
    assert np.array_equal(ids, np.asarray(ev._run.flat.dt_id))
    assert np.array_equal(types, want["dt_type"])
    assert np.array_equal(per["dt_counts"], want["dt_counts"])
    # accumulate() after it: the rows of the pass are as the match left them
    ev.accumulate()
    lines = ev.error_lines(iou_thr, bg_thr)
    assert len(lines) == 2 + n_rng and all(isinstance(x, str) for x in lines)
    assert lines[2].split()[-10:] == [str(int(v)) for v in np.concatenate(
        [want["dt_counts"][0].sum(0), want["gt_counts"][0].sum(0)])]
    return got


@pytest.mark.parametrize("name", ["f1", "f2", "f3", "f4", "f5", "f7", "f9", "f10", "f11"])
def test_class_api_on_the_fixtures(name, tmp_path):
    ev = _tao(name, tmp_path)
    got = _check_class_api(ev, 0.5, 0.1)
    if name in ("f1", "f2", "f4", "f7", "f9"):
        from goldenio import load_eval
        p = load_eval(name)["tao"][0]
        assert np.array_equal(ev.eval["precision"], p)
        assert got["dt_counts"].sum() == 20 * ev._run.dp.n_dt


def test_class_api_at_another_threshold():
    ev = _tao("f1")
    _check_class_api(ev, ev.params.iou_thrs[5], 0.3)


@pytest.mark.parametrize("case,iou_thr", [("few", 0.75), ("few", 0.3), ("ranges3", 0.5)])
def test_class_api_under_edited_constants_of_one_block(case, iou_thr):
    """Thresholds in the caller's unsorted order; 3 area ranges x 2 durations
    (kernel slots 0, 1 and the occlusion one; 0 and 1)."""
    ev = _tao("f1")
    edit(ev.params, cases()[case], "tao")
    got = _check_class_api(ev, iou_thr, 0.1)
    assert got["dt_counts"].shape[0] == len(ev.params.area_rng) * len(ev.params.time_rng)
    if case == "ranges3":
        # a second threshold: the pass evaluate() left out is not run again
        ws = ev._run.ws
        before = ws.err_match_gt.data_ptr(), ws.err_match_gt.clone()
        want = _restated(ev, ev.params.iou_thrs[5], 0.2)
        again = ev.error_types(ev.params.iou_thrs[5], 0.2)
        assert np.array_equal(again["dt_counts"], want["dt_counts"])
        assert np.array_equal(again["gt_counts"], want["gt_counts"])
        assert ws.err_match_gt.data_ptr() == before[0] and bool((ws.err_match_gt == before[1]).all())


def test_class_api_after_accumulate_leaves_the_pass_as_it_was():
    """The usual order: evaluate(), accumulate(), then a first error_types() --
    which runs the match once more for its indices.  The rows, eval["precision"]
    and the eval["scores"] computed afterwards are those of before."""
    ref_ev = _tao("f1")
    ref_ev.evaluate()
    ref_ev.accumulate()
    scores = ref_ev.score_at_recall().copy()
    ev = _tao("f1")
    ev.evaluate()
    ev.accumulate()
    rows = ev._run.ws.rows.clone()
    precision = ev.eval["precision"].copy()
    want = _restated(ev, 0.5, 0.1)
    got = ev.error_types(0.5, 0.1, per_detection=True)
    assert np.array_equal(got["dt_counts"], want["dt_counts"])
    assert np.array_equal(got["gt_counts"], want["gt_counts"])
    assert np.array_equal(got["dt_type"][1], want["dt_type"])
    assert bool((ev._run.ws.rows == rows).all())
    assert np.array_equal(ev.eval["precision"], precision)
    assert np.array_equal(precision, ref_ev.eval["precision"])
    assert np.array_equal(ev.score_at_recall(), scores)
    assert (scores > 0).any()


def test_class_api_on_a_params_subset():
    """params.vid_ids / cat_ids edited: the tables are those of the remaining
    videos, the category axis is in the caller's order."""
    ev = _tao("f1")
    ev.params.vid_ids = ev.params.vid_ids[::2]
    ev.params.cat_ids = [ev.params.cat_ids[i] for i in (4, 0, 2)]
    whole = _tao("f1")
    whole.evaluate()
    got = _check_class_api(ev, 0.5, 0.1)
    assert got["dt_counts"].shape[1] == 3 and got["dt_counts"].sum() > 0
    assert ev._run.dp.n_dt < whole._run.dp.n_dt


def test_class_api_refusals():
    ev = _tao("f1")
    ev.evaluate()
    with pytest.raises(ValueError, match="not one of params.iou_thrs"):
        ev.error_types(0.55000001)
    for bad in (0.5, 0.7, -0.1):
        with pytest.raises(ValueError, match="bg_thr"):
            ev.error_types(0.5, bad)
    from tao_amodal_amd import engine
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_track_error_types(ev._run.dp, ev._run.ws, 10, 0.1)
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_track_error_types(ev._run.dp, ev._run.ws, 0, 0.5)
    with pytest.raises(_lib.TaoAmdError, match="track level's"):
        engine.stage_track_error_types(_lvis_run().dp, _lvis_run().ws, 0, 0.1)
    many = _tao("f1")
    edit(many.params, cases()["many"], "tao")
    many.evaluate()
    with pytest.raises(NotImplementedError, match=r"error_types\(\) is kept for up to 10 IoU"):
        many.error_types(many.params.iou_thrs[9])
    wide = _tao("f1")
    edit(wide.params, cases()["ranges8"], "tao")
    wide.evaluate()
    with pytest.raises(NotImplementedError, match="one block of ranges"):
        wide.error_types(0.5)
    pooled = _tao("f1")
    pooled.params.use_cats = 0
    pooled.evaluate()
    with pytest.raises(NotImplementedError, match="use_cats = 0"):
        pooled.error_types(0.5)
    avg = _tao("f1", iou_3d_type="avg_iou")
    avg.evaluate()
    with pytest.raises(NotImplementedError, match="iou_3d_type='avg_iou'"):
        avg.error_types(0.5)
    with pytest.raises(_lib.TaoAmdError, match="3d_iou"):
        engine.stage_track_error_types(avg._run.dp, avg._run.ws, 0, 0.1)
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval
    segm = TaoEval(Tao(path("f6", "gt.json")), path("f6", "pred_rle.json"), iou_type="segm")
    segm.evaluate()
    with pytest.raises(NotImplementedError, match="iou_type='segm'"):
        segm.error_types(0.5)
    with pytest.raises(_lib.TaoAmdError, match="on boxes"):
        engine.stage_track_error_types(segm._run.dp, segm._run.ws, 0, 0.1)


_LVIS_RUN = []


def _lvis_run():
    from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
    if not _LVIS_RUN:
        ev = LVISEval(path("f1", "gt.json"), path("f1", "pred.json"), "bbox")
        ev.evaluate()
        _LVIS_RUN.append(ev)
    return _LVIS_RUN[0]._run


def test_image_level_error_types_are_unchanged():
    """LVISEval.error_types() on f1 against the image-level restatement."""
    import torch
    from tao_amodal_amd import engine
    run = _lvis_run()
    ev = _LVIS_RUN[0]
    ws = engine.Workspace(run.dp, detail=True)
    engine.run_guarded(run.dp, ws, run.flat, upto="match")
    torch.cuda.synchronize()
    mg = ws.match_gt[:run.dp.n_dt].cpu().numpy()
    gt_rng = ws.gt_rng[:run.dp.n_gt].cpu().numpy().view(np.uint32)
    want = img_ref.error_types(run.flat, mg, gt_rng, orclib.thresholds()[0], 0, 0.1)
    got = ev.error_types(0.5, 0.1, per_detection=True)
    assert np.array_equal(got["dt_counts"], want["dt_counts"])
    assert np.array_equal(got["gt_counts"], want["gt_counts"])
    assert np.array_equal(got["dt_type"][1], want["dt_type"])
