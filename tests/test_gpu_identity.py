"""-m gpu: the track-level identity measures (taoamd_track_identity_share,
taoamd_track_identity_assign, engine.stage_track_identity, TaoEval.identity)
against the numpy restatement of tests/identity_ref.py.  The restatement's
overlaps are the C oracle's bbIou, everything else is an integer: the counts are
compared with ==; an assignment is checked for validity and optimality, since
under ties it is not unique."""
import os

import numpy as np
import pytest

import boxpop
import identity_ref as ref
import orclib
import wsguard
from goldenio import path
from tao_amodal_amd import _lib
from test_gpu_association import _device_association

pytestmark = pytest.mark.gpu

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


def _sizes(t, n_df=None, n_gf=None):
    return (int(t.cell_dt_off[-1]), int(t.cell_gt_off[-1]), len(t.cell_dt_off) - 1,
            int(t.cell_iou_off[-1]), int(t.dt_frame_off[-1]) if n_df is None else n_df,
            int(t.gt_frame_off[-1]) if n_gf is None else n_gf)


def _cells(t):
    return [_up(t.cell_dt_off, np.int32), _up(t.cell_gt_off, np.int32),
            _up(t.cell_iou_off, np.int64)]


def _device_share(f, thr, fill=-3):
    """taoamd_track_identity_share on a Flat; the workspace is exactly the size
    reported, behind a guard band; share holds `fill` beforehand."""
    import torch
    lib = _lib.load()
    sizes = _sizes(f, len(f.dt_frame_pos), len(f.gt_frame_pos))
    cols = _cells(f) + [
        _up(f.dt_frame_off, np.int32), _up(f.dt_frame_pos, np.int32),
        _up(np.asarray(f.dt_frame_box, dtype=np.float64).reshape(-1, 4), np.float64),
        _up(f.gt_frame_off, np.int32), _up(f.gt_frame_pos, np.int32),
        _up(np.asarray(f.gt_frame_box, dtype=np.float64).reshape(-1, 4), np.float64)]
    share = torch.full((max(sizes[3], 1),), fill, dtype=torch.int32, device=DEV)
    ws = wsguard.Guarded(lib.taoamd_track_identity_workspace(sizes[0], sizes[1], sizes[5]), DEV)
    _lib.check(lib.taoamd_track_identity_share(
        *sizes, thr, *[c.data_ptr() for c in cols], share.data_ptr(), ws.data_ptr(), ws.nbytes,
        _stream()), "taoamd_track_identity_share")
    ws.check()
    return share[:sizes[3]].cpu().numpy()


def _device_assign(t, share, fill=-3):
    """taoamd_track_identity_assign on a table (a Flat or identity_ref.table) and
    a share matrix; workspace and outputs as above.  Returns dict(cat_counts,
    gt_ident, dt_ident, status)."""
    import torch
    lib = _lib.load()
    sizes = _sizes(t)
    K = len(t.cat_ids)
    cols = _cells(t) + [_up(t.gt_cat, np.int32), _up(t.gt_flags, np.uint8),
                        _up(t.dt_cat, np.int32), _up(t.dt_flags, np.uint8),
                        _up(t.dt_frame_off, np.int32), _up(t.gt_frame_off, np.int32),
                        _up(share, np.int32)]
    cat_counts = torch.full((K, 6), fill, dtype=torch.int64, device=DEV)
    gt_ident = torch.full((max(sizes[1], 1), 2), fill, dtype=torch.int32, device=DEV)
    dt_ident = torch.full((max(sizes[0], 1), 2), fill, dtype=torch.int32, device=DEV)
    status = torch.full((1,), fill, dtype=torch.int32, device=DEV)
    ws = wsguard.Guarded(lib.taoamd_track_identity_workspace(sizes[0], sizes[1], sizes[5]), DEV)
    _lib.check(lib.taoamd_track_identity_assign(
        *sizes, K, *[c.data_ptr() for c in cols], cat_counts.data_ptr(), gt_ident.data_ptr(),
        dt_ident.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.nbytes, _stream()),
        "taoamd_track_identity_assign")
    ws.check()
    return dict(cat_counts=cat_counts.cpu().numpy(), gt_ident=gt_ident[:sizes[1]].cpu().numpy(),
                dt_ident=dt_ident[:sizes[0]].cpu().numpy(), status=int(status.item()))


def _check(t, share, got, want):
    assert got["status"] == 0
    assert got["cat_counts"].dtype == np.int64
    assert np.array_equal(got["cat_counts"], want["cat_counts"])
    ref.check_assignment(t, share, want, got["gt_ident"], got["dt_ident"])


# ---------------------------------------------------------------------------
# the assignment kernel alone, on synthetic share matrices
# ---------------------------------------------------------------------------
# one cell per (rows, columns), both orientations: nothing, one, two, the sizes
# around a wavefront, and 257 > the 256 columns whose search state fits in LDS;
# (3, 256) is the last that does
SIDES = [(r, c) for r in (0, 1, 2, 63, 64, 65) for c in (0, 1, 63, 64, 65, 257)] + [(3, 256)]
SHAPES = sorted(set(SIDES) | {(c, r) for r, c in SIDES})
N_CAT = 3
FAMILIES = ["dense", "sparse", "equal", "permutation", "zero_row_and_column", "large",
            "ignore_flags", "unmatched_flags"]


def _family(name, seed):
    """(table, share) of one weight family over SHAPES."""
    rng = np.random.default_rng(seed)
    n_dt, n_gt = sum(d for d, _ in SHAPES), sum(g for _, g in SHAPES)
    # two cells' categories lie outside [0, N_CAT): they count nowhere
    cat = [c % N_CAT for c in range(len(SHAPES))]
    cat[5], cat[-3] = N_CAT, -1
    gt_flags, dt_flags = np.zeros(n_gt, np.uint8), np.zeros(n_dt, np.uint8)
    if name == "ignore_flags":
        gt_flags = (rng.random(n_gt) < 0.3).astype(np.uint8)
        gt_flags |= (rng.integers(0, 2, n_gt) * 2).astype(np.uint8)        # another flag: no matter
    if name == "unmatched_flags":
        dt_flags = (rng.random(n_dt) < 0.5).astype(np.uint8)
        dt_flags |= (rng.integers(0, 2, n_dt) * 2).astype(np.uint8)
    t = ref.table(SHAPES, cat, gt_flags, dt_flags, N_CAT, rng)
    parts = []
    for D, G in SHAPES:
        if name in ("dense", "ignore_flags"):
            w = rng.integers(0, 10, (D, G))
        elif name in ("sparse", "unmatched_flags"):
            w = rng.integers(1, 10, (D, G)) * (rng.random((D, G)) < 0.1)
        elif name == "equal":
            w = np.full((D, G), 7)
        elif name == "permutation":
            w = rng.integers(0, 4, (D, G))
            n = min(D, G)
            w[rng.permutation(D)[:n], rng.permutation(G)[:n]] += rng.integers(1000, 2000, n)
        elif name == "zero_row_and_column":
            w = rng.integers(0, 10, (D, G))
            w[:1], w[:, :1] = 0, 0
        else:
            w = rng.integers(0, 2 ** 30 + 1, (D, G))
            w.flat[:1] = 2 ** 30
        parts.append(np.asarray(w, np.int32).ravel())
    return t, np.concatenate(parts).astype(np.int32)


@pytest.mark.parametrize("name", FAMILIES)
def test_assign_on_synthetic_share_matrices(name):
    t, share = _family(name, 11 + FAMILIES.index(name))
    assert int(np.diff(t.cell_dt_off).max()) == 257 == int(np.diff(t.cell_gt_off).max())
    want = ref.identity_from_share(t, share)
    # the family holds what it is for
    if name == "large":
        assert share.max() == 2 ** 30 and want["cat_counts"][:, 4].max() > 2 ** 32
    if name == "ignore_flags":
        assert not want["eligible"].all() and not want["kept"].all()
    if name == "unmatched_flags":
        assert not want["kept"].all() and (want["kept"] & (t.dt_flags & 1 != 0)).any()
    if name == "equal":
        assert want["cell_idtp"].max() == 7 * 65
    got = _device_assign(t, share)
    _check(t, share, got, want)
    again = _device_assign(t, share, fill=77)
    for k in ("cat_counts", "gt_ident", "dt_ident"):
        assert np.array_equal(again[k], got[k]), k
    assert again["status"] == 0


# ---------------------------------------------------------------------------
# the share kernel on seeded tables
# ---------------------------------------------------------------------------
DTS = [0, 1, 63, 64, 65, 257]
GTS = [0, 1, 63, 64, 65]
CELLS = [(d, g) for d in DTS for g in GTS]
# "crowd" cells: ground truths and detections coincide, the matrix is dense
CROWDS = [(65, 64, 5), (20, 20, 30)]          # (detection tracks, ground truths, frames)
LENGTHS = [1, 7, 8, 9, 64, 65, 257]
LENGTH_P = [0.3, 0.2, 0.15, 0.15, 0.1, 0.07, 0.03]
TIMELINE = 300


def _seeded_table(seed, boxes=None):
    """A video per entry of CELLS; its cell of category v % N_CAT holds that many
    tracks.  Tracks of LENGTHS frames with holes on a timeline of 300 positions;
    about half the detection tracks are drifting copies of parts of a ground
    truth, some lie behind the timeline and share no frame.  Then the CROWDS.
    Integer boxes that move by a pixel, or `boxes(n)`: n pairs (detection's side,
    ground truth's side) of any double."""
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

    dets, gts = [], []
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
        for j in range(nd):
            r = rng.random()
            pos, fr = positions(TIMELINE), None
            if r < 0.15:
                pos = np.unique(TIMELINE + pos % 50)  # shares no frame with a ground truth
            if ng and r >= 0.4:
                gpos, gfr, gpop = mine[int(rng.integers(ng))]
                keep = rng.random(len(gpos)) < rng.choice([0.3, 0.6, 1.0])
                keep = keep if keep.any() else np.ones(len(gpos), bool)
                pos = gpos[keep]
                if boxes is None:
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
            dets.append((v, cat, fr, float(rng.integers(0, 20)) / 20,
                         int(rng.choice([0, 0, 1, 2]))))
    for i, (nd, ng, n) in enumerate(CROWDS):
        v, cat = len(CELLS) + i, i % N_CAT
        for _ in range(ng):
            gts.append((v, cat, {p: [int(rng.integers(0, 2)), 0, 10, 10] for p in range(n)},
                        int(rng.choice([0, 0, 0, 1]))))
        for _ in range(nd):
            dets.append((v, cat, {p: [int(rng.integers(0, 3)), 0, 10, 10] for p in range(n)},
                         float(rng.integers(0, 20)) / 20, int(rng.choice([0, 0, 1]))))
    f, _, _ = ref.make_track_flat(len(CELLS) + len(CROWDS), N_CAT, dets, gts)
    return f


@pytest.fixture(scope="module")
def seeded():
    """(flat, {frame_thr: the restated share}), computed once."""
    f = _seeded_table(41)
    want = {thr: ref.share(f, thr) for thr in (0.5, 1.0)}
    for w in want.values():
        w.setflags(write=False)
    return f, want


@pytest.mark.parametrize("thr", [0.5, 1.0])
def test_share_on_the_seeded_table(seeded, thr):
    f, want = seeded
    w = want[thr]
    # the cases are there: every cell shape and track length, holes, crowds
    shapes = set(zip(np.diff(f.cell_dt_off).tolist(), np.diff(f.cell_gt_off).tolist()))
    assert all((d, g) in shapes for d, g in CELLS if d or g)
    assert all((d, g) in shapes for d, g, _ in CROWDS)
    for off in (f.dt_frame_off, f.gt_frame_off):
        assert set(LENGTHS) <= set(np.diff(off).tolist())
    assert (np.diff(f.gt_frame_pos)[np.diff(f.gt_frame_pos) > 0] > 1).any()
    by_cell = list(zip(np.diff(f.cell_dt_off).tolist(), np.diff(f.cell_gt_off).tolist()))
    k = by_cell.index(CROWDS[1][:2])
    crowd = w[f.cell_iou_off[k]:f.cell_iou_off[k + 1]]
    assert (crowd > 0).mean() > 0.9
    assert w.max() > 64 and ((w > 0) & (w < 5)).any()
    got = _device_share(f, thr)
    assert got.dtype == np.int32 and np.array_equal(got, w)
    # elementwise at least the association's follow on the same table
    vis = np.zeros(len(f.gt_frame_pos))
    follow = _device_association(f, vis, thr, vis_rng=[], with_iou=False)["follow"]
    assert (got >= follow).all() and (got > follow).any()
    # and through the assignment: the whole pass on one table
    want_id = ref.identity_from_share(f, w)
    _check(f, w, _device_assign(f, got), want_id)
    assert np.array_equal(_device_share(f, thr, fill=77), got)


def test_share_on_boxes_that_are_any_double():
    """Coordinates from every population of tests/boxpop.py (NaN, +-inf, 1e-160 to
    1e300, negative w and h) against the reference's own compiled bbIou where
    oracle/_ref is built: a NaN overlap is no overlap."""
    prng = np.random.default_rng(79)
    turn = [0]

    def boxes(n):
        kind = boxpop.KINDS[turn[0] % len(boxpop.KINDS)]
        turn[0] += 1
        return boxpop.box_population(kind, 2 * n, prng)
    f = _seeded_table(94, boxes)
    bb = orclib.ref_bb_iou if os.path.exists(orclib.REF_SO) else orclib.bb_iou
    want = ref.share(f, 0.3, bb_iou=bb)
    with np.errstate(all="ignore"):
        every = bb(np.asarray(f.dt_frame_box)[:2000], np.asarray(f.gt_frame_box)[:2000])
    assert np.isnan(every).any() and (want > 0).any()
    assert np.array_equal(_device_share(f, 0.3), want)


@pytest.mark.parametrize("case", ["no_detection_tracks", "no_ground_truth", "no_cells",
                                  "no_detection_frames", "mixed"])
def test_share_on_empty_sides(case):
    """A side without rows, cells or frames, and rows and frames that nothing
    lists (association_ref.empty_sides): share is the restatement's whatever is
    empty, over the frame index the association builds as well."""
    import association_ref
    f, vis = association_ref.empty_sides()[case]
    want = ref.share(f, 0.5)
    got = _device_share(f, 0.5)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if case != "mixed":
        assert not want.any()
        return
    # [the whole track, none, the holed one] x [the long ground truth]; the other cell
    assert want.tolist() == [10, 0, 20, 2]
    # the two passes read one index: a follower shares the frame it follows, and a
    # covered frame is shared by someone
    a = _device_association(f, vis, 0.5)
    assert (a["follow"] <= got).all()
    for c in range(f.n_cells):
        D = f.cell_dt_off[c + 1] - f.cell_dt_off[c]
        g0, g1 = f.cell_gt_off[c], f.cell_gt_off[c + 1]
        column = got[f.cell_iou_off[c]:f.cell_iou_off[c + 1]].reshape(D, g1 - g0).sum(0)
        assert (a["gt_assoc"][g0:g1, 1] <= column).all() and a["gt_assoc"][g0:g1, 1].all()


def test_both_calls_on_the_hand_written_table():
    f, dt_at, gt_at = ref.hand_flat()
    for thr, cell1, gi_want, counts in (
            (ref.HAND_THR, ref.HAND_SHARE_CELL1, ref.HAND_GT_IDENT, ref.HAND_CAT_COUNTS),
            (ref.HAND_THR_ABOVE, ref.HAND_SHARE_CELL1_ABOVE, ref.HAND_GT_IDENT_ABOVE,
             ref.HAND_CAT_COUNTS_ABOVE)):
        share = _device_share(f, thr)
        k0, k1 = int(f.gt_cell[gt_at[0]]), int(f.gt_cell[gt_at[2]])
        assert share[f.cell_iou_off[k0]:f.cell_iou_off[k0 + 1]].reshape(2, 2).tolist() \
            == ref.HAND_SHARE_CELL0
        assert share[f.cell_iou_off[k1]:f.cell_iou_off[k1 + 1]].reshape(3, 2).tolist() == cell1
        assert np.array_equal(share, ref.share(f, thr))
        got = _device_assign(f, share)
        assert got["status"] == 0 and got["cat_counts"].tolist() == counts
        gi, di = ref.by_given(got, dt_at, gt_at)       # (the optimum is unique here)
        assert gi == gi_want and di == ref.HAND_DT_IDENT
        _check(f, share, got, ref.identity_from_share(f, share))


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


@pytest.mark.parametrize("name", ["f1", "f4"])
def test_class_api_on_the_fixtures(name):
    ev = _tao(name)
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.identity()
    ev.evaluate()
    ev.accumulate()
    before = {k: ev.eval[k].copy() for k in ("precision", "recall")}
    flat = ev._run.flat
    want = ref.identity(flat, 0.5)
    cats = np.asarray(flat.cat_ids).tolist()
    pos = [cats.index(int(c)) for c in ev.params.cat_ids]
    got = ev.identity()
    K = len(ev.params.cat_ids)
    assert "tracks" not in got and "dt_tracks" not in got
    assert got["columns"] == list(ref.CAT_COLUMNS) and got["frame_thr"] == 0.5
    assert got["cat_counts"].shape == (K, 6) and got["cat_counts"].dtype == np.int64
    assert np.array_equal(got["cat_counts"], want["cat_counts"][pos])
    idf1, idp, idr = ref.ratios(want["cat_counts"][pos])
    for key, w in (("idf1", idf1), ("idp", idp), ("idr", idr)):
        assert got[key].dtype == np.float64 and np.array_equal(got[key], w, equal_nan=True), key
    tot = got["total"]
    sums = want["cat_counts"].sum(0)
    assert [tot[c] for c in ref.CAT_COLUMNS] == sums.tolist() and tot["idtp"] > 0
    assert tot["idfn"] == sums[1] - sums[4] and tot["idfp"] == sums[3] - sums[4]
    assert tot["idf1"] == 2 * sums[4] / (sums[1] + sums[3])
    assert tot["idp"] == sums[4] / sums[3] and tot["idr"] == sums[4] / sums[1]
    # one to one can explain no more frames than many to one covers
    assert tot["idtp"] <= ev.association()["cat_counts"][:, 2].sum()
    assert ev.identity()["cat_counts"] is got["cat_counts"]                   # cached
    full = ev.identity(per_track=True)
    assert full["cat_counts"] is got["cat_counts"]
    gt_ids, tracks = full["tracks"]
    dt_ids, dt_tracks = full["dt_tracks"]
    assert np.array_equal(gt_ids, np.asarray(flat.gt_id)) and tracks.dtype == np.int64
    assert np.array_equal(dt_ids, np.asarray(flat.dt_id)) and dt_tracks.dtype == np.int64
    assert np.array_equal(tracks[:, 2], np.diff(flat.gt_frame_off))
    assert np.array_equal(dt_tracks[:, 2], np.diff(flat.dt_frame_off))
    assert np.array_equal(dt_tracks[:, 1], want["kept"].astype(np.int64))
    # ids back to rows: a valid and optimal assignment
    d_row = {int(i): r for r, i in enumerate(np.asarray(flat.dt_id))}
    g_row = {int(i): r for r, i in enumerate(np.asarray(flat.gt_id))}
    gi = np.array([[d_row.get(int(a), -1), b] for a, b, _ in tracks], np.int32).reshape(-1, 2)
    di = np.array([[g_row.get(int(a), -1), b] for a, b, _ in dt_tracks], np.int32).reshape(-1, 2)
    ref.check_assignment(flat, want["share"], want, gi, di)
    assert tracks[:, 1].sum() == tot["idtp"]
    lines = ev.identity_lines()
    assert len(lines) == 3 and all(isinstance(x, str) and x for x in lines)
    assert "IDF1" in lines[1] and "idtp={}".format(tot["idtp"]) in lines[2]
    # another threshold: another table under another key
    one = ev.identity(1.0)
    assert np.array_equal(one["cat_counts"], ref.identity(flat, 1.0)["cat_counts"][pos])
    assert one["total"]["idtp"] <= tot["idtp"] and one["frame_thr"] == 1.0
    # nothing of the evaluation moved
    for k, v in before.items():
        assert np.array_equal(ev.eval[k], v, equal_nan=True), k


def test_class_api_refusals():
    ev = _tao("f1")
    ev.evaluate()
    for bad in (0.0, -0.1, 1 + 2.0 ** -52, float("nan")):
        with pytest.raises(ValueError, match="frame_thr"):
            ev.identity(bad)
    from tao_amodal_amd import engine
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_track_identity(ev._run.dp, ev._run.ws, 0.0)
    pooled = _tao("f1")
    pooled.params.use_cats = 0
    pooled.evaluate()
    with pytest.raises(NotImplementedError, match="use_cats = 0"):
        pooled.identity()
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval
    segm = TaoEval(Tao(path("f6", "gt.json")), path("f6", "pred_rle.json"), iou_type="segm")
    segm.evaluate()
    with pytest.raises(NotImplementedError, match="iou_type='segm'"):
        segm.identity()
    with pytest.raises(_lib.TaoAmdError, match="on boxes"):
        engine.stage_track_identity(segm._run.dp, segm._run.ws, 0.5)
    # a multi-GPU run: its evaluator refuses, and nothing is cached
    from tao_amodal_amd.evaluation._dist import DistRun
    ev._run = DistRun.__new__(DistRun)
    with pytest.raises(NotImplementedError, match=r"identity\(\) in a multi-GPU run"):
        ev.identity()
    with pytest.raises(NotImplementedError, match=r"identity\(\) in a multi-GPU run"):
        ev.identity_lines()
    assert ev._identity == {}
