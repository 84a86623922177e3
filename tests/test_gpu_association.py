"""-m gpu: the track-level association (taoamd_track_association,
engine.stage_track_association, TaoEval.association) against the numpy
restatement of tests/association_ref.py.  The restatement's overlaps are the C
oracle's bbIou, everything else is an integer: every comparison is exact."""
import os
import sys

import numpy as np
import pytest

import association_ref as ref
import boxpop
import orclib
import wsguard
from goldenio import GOLDEN as GOLDEN_DIR, path
from tao_amodal_amd import _lib

sys.path.insert(0, GOLDEN_DIR)
from constants_cases import cases, edit  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = _lib.TRACK_ASSOCIATION_TILE
DEV = "cuda:0"
KEYS = ("follow", "gt_assoc", "cat_counts", "vis_counts", "best", "best_iou")


def _up(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], dtype=dtype)
    return torch.from_numpy(a).to(DEV)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _device_association(f, vis, thr, vis_rng=ref.VIS_RNG, status=False, ws_bytes=None,
                        with_iou=True, fill=-3):
    """taoamd_track_association on a Flat; the workspace is exactly the size
    reported, behind a guard band; the outputs hold `fill` beforehand."""
    import torch
    lib = _lib.load()
    n_dt, n_gt, K = int(f.cell_dt_off[-1]), int(f.cell_gt_off[-1]), len(f.cat_ids)
    n_iou, n_df, n_gf = int(f.cell_iou_off[-1]), len(f.dt_frame_pos), len(f.gt_frame_pos)
    vis_rng = np.asarray(vis_rng, dtype=np.float64).reshape(-1, 2)
    n_vis = len(vis_rng)
    cols = [_up(f.cell_dt_off, np.int32), _up(f.cell_gt_off, np.int32),
            _up(f.cell_iou_off, np.int64), _up(f.gt_cat, np.int32), _up(f.gt_flags, np.uint8),
            _up(f.dt_frame_off, np.int32), _up(f.dt_frame_pos, np.int32),
            _up(np.asarray(f.dt_frame_box, dtype=np.float64).reshape(-1, 4), np.float64),
            _up(f.gt_frame_off, np.int32), _up(f.gt_frame_pos, np.int32),
            _up(np.asarray(f.gt_frame_box, dtype=np.float64).reshape(-1, 4), np.float64)]
    vis_t, rng_t = _up(vis, np.float64), _up(vis_rng, np.float64)
    follow = torch.full((max(n_iou, 1),), fill, dtype=torch.int32, device=DEV)
    gt_assoc = torch.full((max(n_gt, 1), 7), fill, dtype=torch.int32, device=DEV)
    cat_counts = torch.full((K, 8), fill, dtype=torch.int64, device=DEV)
    vis_counts = torch.full((max(n_vis, 1), K, 3), fill, dtype=torch.int64, device=DEV)
    best = torch.full((max(n_gf, 1),), fill, dtype=torch.int32, device=DEV)
    best_iou = torch.full((max(n_gf, 1),), float(fill), dtype=torch.float64, device=DEV)
    need = lib.taoamd_track_association_workspace(n_dt, n_gt, n_gf)
    ws = wsguard.Guarded(need if ws_bytes is None else ws_bytes, DEV)
    st = lib.taoamd_track_association(
        n_dt, n_gt, f.n_cells, n_iou, n_df, n_gf, K, n_vis, thr,
        *[c.data_ptr() for c in cols], vis_t.data_ptr() if n_vis else None,
        rng_t.data_ptr() if n_vis else None, follow.data_ptr(), gt_assoc.data_ptr(),
        cat_counts.data_ptr(), vis_counts.data_ptr() if n_vis else None, best.data_ptr(),
        best_iou.data_ptr() if with_iou else None, ws.data_ptr(), ws.nbytes, _stream())
    if status:
        torch.cuda.synchronize()
        return st
    _lib.check(st, "taoamd_track_association")
    ws.check()
    return dict(follow=follow[:n_iou].cpu().numpy(), gt_assoc=gt_assoc[:n_gt].cpu().numpy(),
                cat_counts=cat_counts.cpu().numpy(), vis_counts=vis_counts[:n_vis].cpu().numpy(),
                best=best[:n_gf].cpu().numpy(),
                best_iou=best_iou[:n_gf].cpu().numpy() if with_iou else None)


def _same(got, want):
    for k in KEYS:
        if got[k] is not None:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert np.array_equal(got[k], want[k]), k


def test_abi_on_the_hand_written_table():
    f, dt_at, gt_at, vis = ref.hand_flat()
    got = _device_association(f, vis, ref.HAND_THR)
    rows = got["gt_assoc"][gt_at].astype(np.int64)
    assert rows[:, :5].tolist() == [r[:5] for r in ref.HAND_ASSOC]
    assert rows[:, 5].tolist() == [dt_at[r[5]] if r[5] >= 0 else -1 for r in ref.HAND_ASSOC]
    assert rows[:, 6].tolist() == [r[6] for r in ref.HAND_ASSOC]
    s = int(f.gt_frame_off[gt_at[0]])
    assert got["best"][s:s + 6].tolist() == ref.HAND_BEST_GT0
    assert got["best_iou"][s:s + 6].tolist() == ref.HAND_BEST_IOU_GT0
    k = int(f.gt_cell[gt_at[0]])
    assert got["follow"][f.cell_iou_off[k]:f.cell_iou_off[k + 1]].reshape(2, 2).tolist() \
        == ref.HAND_FOLLOW_CELL0
    assert got["cat_counts"].tolist() == ref.HAND_CAT_COUNTS
    assert got["vis_counts"][:, 0].tolist() == ref.HAND_VIS_COUNTS
    _same(got, ref.association(f, vis, ref.HAND_THR))
    # an overlap of exactly frame_thr covers; two units in the last place above, it does not
    up = _device_association(f, vis, ref.HAND_THR_ABOVE)
    assert up["gt_assoc"][gt_at[2], :5].tolist() == ref.HAND_ASSOC_ABOVE_GT2[:5]
    assert up["cat_counts"].tolist() == ref.HAND_CAT_COUNTS_ABOVE
    _same(up, ref.association(f, vis, ref.HAND_THR_ABOVE))
    # no windows, no best_iou: the rest is the same
    bare = _device_association(f, vis, ref.HAND_THR, vis_rng=[], with_iou=False)
    assert bare["vis_counts"].shape == (0, 2, 3) and bare["best_iou"] is None
    for key in ("follow", "gt_assoc", "cat_counts", "best"):
        assert np.array_equal(bare[key], got[key])


# (detection tracks, ground-truth tracks) per cell: every pairing of the sizes
# around a wavefront / a workgroup of the follow-up kernels and around the pair
# kernel's tile of ground-truth frames (tracks of one frame make a tile of tracks)
DTS = [0, 1, 63, 64, 65, 257]
GTS = sorted({0, 1, TILE - 1, TILE, TILE + 1})
CELLS = [(d, g) for d in DTS for g in GTS]
N_CAT = 3
LENGTHS = [1, 7, 8, 9, 64, 65, 257]
LENGTH_P = [0.3, 0.2, 0.15, 0.15, 0.1, 0.07, 0.03]
TIMELINE = 300


def _seeded_table(seed, boxes=None):
    """A video per entry of CELLS; its cell of category v % N_CAT holds that many
    tracks, a neighbouring category a few detection tracks that lie on the
    ground truths.  Tracks of LENGTHS frames with holes on a timeline of 300
    positions; detection tracks behind it share no frame with a ground truth.
    Integer boxes that move by a pixel, or `boxes(n)`: n pairs (detection's
    side, ground truth's side) of any double.  Returns (flat, vis)."""
    rng = np.random.default_rng(seed)

    def positions(top):
        n = min(int(rng.choice(LENGTHS, p=LENGTH_P)), top)
        span = min(top, n + int(rng.integers(0, n + 1)))
        lo = int(rng.integers(0, top - span + 1))
        return np.sort(lo + rng.choice(span, n, replace=False))

    def box():
        x, y = rng.integers(0, 6, 2) * 4
        w, h = rng.choice([4, 8, 16], 2)
        return [int(x), int(y), int(w), int(h)]

    dets, gts, vis = [], [], []
    for v, (nd, ng) in enumerate(CELLS):
        cat = v % N_CAT
        mine = []
        for _ in range(ng):
            pos = positions(TIMELINE)
            if boxes is None:
                bx = box()
                fr = {int(p): [bx[0] + int(rng.integers(0, 2)), bx[1], bx[2], bx[3]] for p in pos}
                pop = None
            else:
                pop = boxes(len(pos))
                fr = {int(p): pop[2 * k + 1].tolist() for k, p in enumerate(pos)}
            mine.append((pos, fr, pop))
            gts.append((v, cat, fr, int(rng.choice([0, 0, 0, 1]))))
            vis.append({int(p): float(rng.choice([0.0, 0.05, 0.1, 0.5, 0.8, 0.9, 1.0, np.nan]))
                        for p in pos})
        for j in range(nd + (3 if ng else 0)):
            other = j >= nd                           # another category, on a ground truth
            r = rng.random()
            pos, fr = positions(TIMELINE), None
            if r < 0.15:
                pos = np.unique(TIMELINE + pos % 50)  # shares no frame with a ground truth
            if ng and (other or r >= 0.4):
                gpos, gfr, gpop = mine[int(rng.integers(ng))]
                keep = rng.random(len(gpos)) < rng.choice([0.3, 0.6, 1.0])
                keep = keep if keep.any() else np.ones(len(gpos), bool)
                pos = gpos[keep]
                if boxes is None:
                    # a copy that drifts: IoUs around the threshold, equal ones among copies
                    dx = int(rng.integers(0, 3))
                    fr = {int(p): [gfr[int(p)][0] + dx * int(rng.integers(0, 2)),
                                   gfr[int(p)][1], gfr[int(p)][2], gfr[int(p)][3]] for p in pos}
                else:
                    fr = {int(p): gpop[2 * k].tolist() for k, p in zip(np.flatnonzero(keep), pos)}
            if fr is None:
                if boxes is None:
                    bx = box()
                    fr = {int(p): bx for p in pos}
                else:
                    pop = boxes(len(pos))
                    fr = {int(p): pop[2 * k].tolist() for k, p in enumerate(pos)}
            dets.append((v, (cat + 1) % N_CAT if other else cat, fr,
                         float(rng.integers(0, 20)) / 20, int(rng.choice([0, 0, 1, 2]))))
    f, _, gt_at = ref.make_track_flat(len(CELLS), N_CAT, dets, gts)
    return f, ref.frame_vis(f, gt_at, vis)


@pytest.fixture(scope="module")
def seeded():
    """(flat, vis, {frame_thr: restatement}), computed once."""
    f, vis = _seeded_table(31)
    want = {thr: ref.association(f, vis, thr) for thr in (0.5, 1.0)}
    for w in want.values():
        for v in w.values():
            v.setflags(write=False)
    return f, vis, want


@pytest.mark.parametrize("thr", [0.5, 1.0])
def test_abi_on_the_seeded_table(seeded, thr):
    f, vis, want = seeded
    w = want[thr]
    # the cases are there: every cell shape and track length, holes, long timelines,
    # switches, fragments, equal counts, tracks that share no frame, NaN visibilities
    shapes = set(zip(np.diff(f.cell_dt_off).tolist(), np.diff(f.cell_gt_off).tolist()))
    assert all((d, g) in shapes for d, g in CELLS if d or g)
    for off in (f.dt_frame_off, f.gt_frame_off):
        assert set(LENGTHS) <= set(np.diff(off).tolist())
    assert int(f.dt_frame_pos.max()) >= 290 and int(f.gt_frame_pos.max()) >= 240
    assert (np.diff(f.gt_frame_pos)[np.diff(f.gt_frame_pos) > 0] > 1).any()
    assert int(np.diff(f.gt_frame_off).max()) > 256 and len(f.gt_frame_pos) > 64 * 256
    assert np.isnan(vis).any() and (vis == 0.1).any() and (vis == 0.8).any()
    if thr == 0.5:
        a = w["gt_assoc"]
        assert (a[:, 3] > 2).any() and (a[:, 4] > 2).any() and (a[:, 2] > 2).any()
        assert (a[:, 1] == 0).any() and (a[:, 1] == a[:, 0]).any()
        assert ((w["best"] < 0) & (w["best_iou"] == 0)).any() and (w["best"] > 64).any()
        assert w["cat_counts"][:, 6].all() and w["cat_counts"][:, 7].all()
    assert (w["vis_counts"][..., 2] < w["vis_counts"][..., 1]).any() or thr == 1.0
    got = _device_association(f, vis, thr)
    _same(got, w)
    # the stated consequence: a track's column of follow adds up to its covered frames
    for c in range(f.n_cells):
        D = f.cell_dt_off[c + 1] - f.cell_dt_off[c]
        G = f.cell_gt_off[c + 1] - f.cell_gt_off[c]
        if D and G:
            m = got["follow"][f.cell_iou_off[c]:f.cell_iou_off[c + 1]].reshape(D, G)
            assert np.array_equal(m.sum(0), got["gt_assoc"][f.cell_gt_off[c]:f.cell_gt_off[c + 1], 1])


def test_abi_does_not_depend_on_arrival_order(seeded, monkeypatch):
    """The same table twice, over outputs that held different values, and once
    with the workspace base moved by 8 bytes (the entry point takes the cells'
    rows as the table has them: there is no row list to reorder).  Every output
    is identical."""
    f, vis, want = seeded
    one = _device_association(f, vis, 0.5)
    two = _device_association(f, vis, 0.5, fill=77)
    monkeypatch.setattr(wsguard, "SHIFT", 8)
    three = _device_association(f, vis, 0.5, fill=-1)
    for other in (two, three):
        _same(other, one)
    _same(one, want[0.5])


def test_abi_on_boxes_that_are_any_double():
    """Coordinates from every population of tests/boxpop.py (NaN, +-inf, 1e-160 to
    1e300, negative w and h) against the reference's own compiled bbIou where
    oracle/_ref is built: a NaN overlap covers nothing."""
    prng = np.random.default_rng(78)
    turn = [0]

    def boxes(n):
        kind = boxpop.KINDS[turn[0] % len(boxpop.KINDS)]
        turn[0] += 1
        return boxpop.box_population(kind, 2 * n, prng)
    f, vis = _seeded_table(93, boxes)
    bb = orclib.ref_bb_iou if os.path.exists(orclib.REF_SO) else orclib.bb_iou
    want = ref.association(f, vis, 0.3, bb_iou=bb)
    with np.errstate(all="ignore"):
        every = bb(np.asarray(f.dt_frame_box)[:2000], np.asarray(f.gt_frame_box)[:2000])
    assert np.isnan(every).any()
    assert (want["best"] >= 0).any() and (want["best_iou"] > 0.3).any()
    got = _device_association(f, vis, 0.3)
    assert not np.isnan(got["best_iou"]).any()
    _same(got, want)


@pytest.mark.parametrize("case", ["no_detection_tracks", "no_ground_truth", "no_cells",
                                  "no_detection_frames", "mixed"])
def test_abi_on_empty_sides(case):
    """A side without rows, cells or frames, and rows and frames that nothing
    lists (association_ref.empty_sides): the frame index is complete whatever is
    empty, and every output is the restatement's."""
    f, vis = ref.empty_sides()[case]
    want = ref.association_of_table(f, vis, 0.5)
    if case == "mixed":
        # the hole is probed, both followers of the long track are found
        assert want["gt_assoc"][1].tolist() == [65, 20, 2, 1, 2, 0, 10]
        assert want["best"][2:2 + 21].tolist() == [0] * 10 + [-1] + [2] * 10
        assert want["gt_assoc"][0].tolist() == [2, 0, 0, 0, 0, -1, 0]
    _same(_device_association(f, vis, 0.5), want)


def test_abi_error_paths():
    f, _, _, vis = ref.hand_flat()
    lib = _lib.load()
    need = lib.taoamd_track_association_workspace(
        int(f.cell_dt_off[-1]), int(f.cell_gt_off[-1]), len(f.gt_frame_pos))
    call = lambda **kw: _device_association(f, vis, kw.pop("thr", 0.5), status=True, **kw)  # noqa: E731
    for bad in (0.0, -0.1, 1 + 2.0 ** -52, float("nan")):
        assert call(thr=bad) == 2
    assert call(vis_rng=[[0, 1]] * 9) == 2
    assert call(ws_bytes=need - 1) == 4
    assert call() == 0 and call(vis_rng=[[0, 1]] * 8) == 0


# ---------------------------------------------------------------------------
# the class API
# ---------------------------------------------------------------------------
def _tao(name, **kw):
    from tao_amodal_amd import flatten
    from tao_amodal_amd.columns import DTColumns
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval, TaoResults
    dt = DTColumns.from_json(path(name, "pred.json"))
    dt.track_id, _ = flatten.make_track_ids_unique(dt)
    gt = Tao(path(name, "gt.json"))
    return TaoEval(gt, TaoResults(gt, dt), **kw)


def _restated(ev, thr, vis_rng=ref.VIS_RNG):
    """The restatement on the evaluator's own tables, the category axis in the
    caller's order, ids for rows."""
    flat = ev._run.flat
    vis = np.asarray(ev._gt_columns.ann_vis, dtype=np.float64)[flat.gt_frame_box.index]
    w = ref.association(flat, vis, thr, vis_rng)
    cats = np.asarray(flat.cat_ids).tolist()
    pos = [cats.index(int(c)) for c in ev.params.cat_ids]
    dt_id, gt_cell = np.asarray(flat.dt_id, np.int64), np.asarray(flat.gt_cell, np.int64)
    tracks = w["gt_assoc"].astype(np.int64)
    tracks[:, 5] = [dt_id[r] if r >= 0 else -1 for r in tracks[:, 5]]
    g_of = np.repeat(np.arange(len(gt_cell)), np.diff(flat.gt_frame_off))
    row = np.asarray(flat.cell_dt_off, np.int64)[gt_cell[g_of]] + w["best"]
    best_id = np.array([dt_id[r] if b >= 0 else -1 for r, b in zip(row, w["best"])], np.int64)
    vid = np.asarray(flat.cell_unit, np.int64)[gt_cell[g_of]]
    img = np.asarray(flat.tl_image_id)[np.asarray(flat.tl_vid_start, np.int64)[vid]
                                       + np.asarray(flat.gt_frame_pos, np.int64)]
    return dict(cat_counts=w["cat_counts"][pos], vis_counts=w["vis_counts"][:, pos],
                tracks=tracks, best_id=best_id, best_iou=w["best_iou"], img=img)


def _check_class_api(ev, thr=0.5):
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.association(thr)
    ev.evaluate()
    ev.accumulate()
    before = {k: ev.eval[k].copy() for k in ("precision", "recall")}
    want = _restated(ev, thr)
    got = ev.association(thr)
    K = len(ev.params.cat_ids)
    assert "tracks" not in got and "frames" not in got
    assert got["columns"]["cat_counts"] == list(ref.CAT_COLUMNS)
    assert got["columns"]["tracks"] == list(ref.TRACK_COLUMNS)
    assert got["vis_rng"] == [[float(a), float(b)] for a, b in ref.VIS_RNG]
    assert got["vis_lbl"] == ["all", "highly-occluded", "partially-occluded", "highly-visible",
                              "highly-and-partially-occluded"]
    assert got["frame_thr"] == thr
    assert got["cat_counts"].shape == (K, 8) and got["cat_counts"].dtype == np.int64
    assert got["vis_counts"].shape == (5, K, 3) and got["vis_counts"].dtype == np.int64
    assert np.array_equal(got["cat_counts"], want["cat_counts"])
    assert np.array_equal(got["vis_counts"], want["vis_counts"])
    assert got["cat_counts"][:, 2].sum() > 0
    assert ev.association(thr)["cat_counts"] is got["cat_counts"]              # cached
    full = ev.association(thr, per_track=True, per_frame=True)
    assert full["cat_counts"] is got["cat_counts"]
    flat = ev._run.flat
    ids, tracks = full["tracks"]
    assert np.array_equal(ids, np.asarray(flat.gt_id)) and np.array_equal(tracks, want["tracks"])
    assert set(tracks[:, 5].tolist()) - {-1} <= set(np.asarray(flat.dt_id).tolist())
    frame_off, img, best_id, best_iou = full["frames"]
    assert np.array_equal(frame_off, np.asarray(flat.gt_frame_off))
    assert np.array_equal(img, want["img"]) and np.array_equal(best_id, want["best_id"])
    assert np.array_equal(best_iou, want["best_iou"])
    # image ids come from the timeline: those of the ground truth's own annotations
    cols = ev._gt_columns
    assert np.array_equal(img, np.asarray(cols.ann_img)[flat.gt_frame_box.index])
    lines = ev.association_lines(thr)
    assert len(lines) == 2 + 5 and all(isinstance(x, str) for x in lines)
    assert lines[2].split()[0] == "all" and lines[2].split()[1] == str(int(want["vis_counts"][0, :, 0].sum()))
    # nothing of the evaluation moved
    for k, v in before.items():
        assert np.array_equal(ev.eval[k], v, equal_nan=True), k
    ev.accumulate()
    for k, v in before.items():
        assert np.array_equal(ev.eval[k], v, equal_nan=True), k
    return got


@pytest.mark.parametrize("name", ["f1", "f11"])
def test_class_api_on_the_fixtures(name):
    ev = _tao(name)
    _check_class_api(ev)
    if name == "f1":
        from goldenio import load_eval
        assert np.array_equal(ev.eval["precision"], load_eval(name)["tao"][0])
        # other arguments: another table under another key
        one = ev.association(1.0, vis_rng=[[0.25, 0.75]], vis_lbl=["mid"])
        want = _restated(ev, 1.0, [[0.25, 0.75]])
        assert np.array_equal(one["cat_counts"], want["cat_counts"])
        assert np.array_equal(one["vis_counts"], want["vis_counts"])
        assert one["vis_lbl"] == ["mid"] and len(ev.association_lines(1.0, [[0.25, 0.75]])) == 3
        none = ev.association(0.5, vis_rng=[])
        assert none["vis_counts"].shape == (0, len(ev.params.cat_ids), 3)
        assert np.array_equal(none["cat_counts"], ev.association(0.5)["cat_counts"])


def test_class_api_on_a_params_subset():
    """params.cat_ids edited: the category axis is in the caller's order."""
    whole = _tao("f1")
    whole.evaluate()
    all_cats = list(whole.params.cat_ids)
    base = whole.association()
    ev = _tao("f1")
    pick = (4, 0, 2)
    ev.params.cat_ids = [ev.params.cat_ids[i] for i in pick]
    got = _check_class_api(ev)
    assert got["cat_counts"].shape[0] == 3
    at = [all_cats.index(c) for c in ev.params.cat_ids]
    assert np.array_equal(got["cat_counts"], base["cat_counts"][at])
    assert np.array_equal(got["vis_counts"], base["vis_counts"][:, at])


def test_class_api_does_not_depend_on_the_constants():
    plain = _tao("f1")
    plain.evaluate()
    base = plain.association(per_track=True, per_frame=True)
    wide = _tao("f1")
    edit(wide.params, cases()["ranges8"], "tao")
    wide.evaluate()
    avg = _tao("f1", iou_3d_type="avg_iou")
    avg.evaluate()
    for ev in (wide, avg):
        got = ev.association(per_track=True, per_frame=True)
        assert np.array_equal(got["cat_counts"], base["cat_counts"])
        assert np.array_equal(got["vis_counts"], base["vis_counts"])
        assert np.array_equal(got["tracks"][1], base["tracks"][1])
        for a, b in zip(got["frames"], base["frames"]):
            assert np.array_equal(a, b)


def test_class_api_refusals():
    ev = _tao("f1")
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.association()
    ev.evaluate()
    for bad in (0.0, -0.1, 1 + 2.0 ** -52, float("nan")):
        with pytest.raises(ValueError, match="frame_thr"):
            ev.association(bad)
    with pytest.raises(ValueError, match="up to 8"):
        ev.association(vis_rng=[[0, 1]] * 9)
    from tao_amodal_amd import engine
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_track_association(ev._run.dp, ev._run.ws, 0.0, [])
    pooled = _tao("f1")
    pooled.params.use_cats = 0
    pooled.evaluate()
    with pytest.raises(NotImplementedError, match="use_cats = 0"):
        pooled.association()
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval
    segm = TaoEval(Tao(path("f6", "gt.json")), path("f6", "pred_rle.json"), iou_type="segm")
    segm.evaluate()
    with pytest.raises(NotImplementedError, match="iou_type='segm'"):
        segm.association()
    with pytest.raises(_lib.TaoAmdError, match="on boxes"):
        engine.stage_track_association(segm._run.dp, segm._run.ws, 0.5, [])
    from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
    img = LVISEval(path("f1", "gt.json"), path("f1", "pred.json"), "bbox")
    img.evaluate()
    with pytest.raises(_lib.TaoAmdError, match="track level's"):
        engine.stage_track_association(img._run.dp, img._run.ws, 0.5, [])
