"""-m gpu: track-level HOTA (taoamd_track_hota_align, taoamd_track_hota_match,
taoamd_track_hota_reduce, engine.stage_track_hota, TaoEval.hota) against the
numpy restatement of tests/hota_ref.py.  Every call goes through the ABI with a
workspace of exactly the reported size behind a guard band and with outputs
pre-filled with junk; every device output is an integer (match_iou: one box_iou
value) and is compared with ==.  The per-frame assignment is checked for
validity and against scipy's optimum on the integer matrix as well."""
import numpy as np
import pytest

import boxpop
import hota_ref as ref
import identity_ref
import orclib
import wsguard
from goldenio import path
from tao_amodal_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ONE = ref.ONE


def _up(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], dtype=dtype)
    return torch.from_numpy(a).to(DEV)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _sizes(t):
    return (int(t.cell_dt_off[-1]), int(t.cell_gt_off[-1]), len(t.cell_dt_off) - 1,
            int(t.cell_iou_off[-1]), len(t.dt_frame_pos), len(t.gt_frame_pos))


def _cells(t):
    return [_up(t.cell_dt_off, np.int32), _up(t.cell_gt_off, np.int32),
            _up(t.cell_iou_off, np.int64)]


def _frames(t):
    return [_up(t.dt_frame_off, np.int32), _up(t.dt_frame_pos, np.int32),
            _up(np.asarray(t.dt_frame_box, dtype=np.float64).reshape(-1, 4), np.float64),
            _up(t.gt_frame_off, np.int32), _up(t.gt_frame_pos, np.int32),
            _up(np.asarray(t.gt_frame_box, dtype=np.float64).reshape(-1, 4), np.float64)]


def _ws(sizes):
    lib = _lib.load()
    return wsguard.Guarded(lib.taoamd_track_hota_workspace(sizes[0], sizes[1], sizes[5]), DEV)


def _keep_ptr(keep, hold):
    if keep is None:
        return None
    hold.append(_up(keep, np.uint8))
    return hold[-1].data_ptr()


def _device_align(t, keep=None, fill=-3):
    import torch
    lib, sizes, hold = _lib.load(), _sizes(t), []
    cols = _cells(t) + [_up(t.gt_flags, np.uint8)]
    pot = torch.full((max(sizes[3], 1),), fill, dtype=torch.int64, device=DEV)
    ws = _ws(sizes)
    _lib.check(lib.taoamd_track_hota_align(
        *sizes, *[c.data_ptr() for c in cols], _keep_ptr(keep, hold),
        *[c.data_ptr() for c in _hold(hold, _frames(t))], pot.data_ptr(), ws.data_ptr(),
        ws.nbytes, _stream()), "taoamd_track_hota_align")
    ws.check()
    return pot[:sizes[3]].cpu().numpy()


def _hold(hold, tensors):
    hold.extend(tensors)
    return tensors


def _device_match(t, pot, alphas, keep=None, fill=-3, with_iou=True):
    import torch
    lib, sizes, hold = _lib.load(), _sizes(t), []
    alphas = np.ascontiguousarray(alphas, np.float64)
    A = len(alphas)
    cols = _cells(t) + [_up(t.gt_flags, np.uint8)]
    mc = torch.full((A, max(sizes[3], 1)), fill, dtype=torch.int32, device=DEV)
    lc = torch.full((A, max(sizes[3], 1)), fill, dtype=torch.int64, device=DEV)
    mt = torch.full((max(sizes[5], 1),), fill, dtype=torch.int32, device=DEV)
    mi = torch.full((max(sizes[5], 1),), float(fill), dtype=torch.float64, device=DEV)
    status = torch.full((1,), fill, dtype=torch.int32, device=DEV)
    ws = _ws(sizes)
    _lib.check(lib.taoamd_track_hota_match(
        *sizes, A, alphas.ctypes.data, *[c.data_ptr() for c in cols], _keep_ptr(keep, hold),
        *[c.data_ptr() for c in _hold(hold, _frames(t))], _up(pot, np.int64).data_ptr(),
        mc.data_ptr(), lc.data_ptr(), mt.data_ptr(), mi.data_ptr() if with_iou else None,
        status.data_ptr(), ws.data_ptr(), ws.nbytes, _stream()), "taoamd_track_hota_match")
    ws.check()
    n = sizes[3]
    return dict(mc=mc.cpu().numpy().reshape(A, -1)[:, :n] if n else np.zeros((A, 0), np.int32),
                lc=lc.cpu().numpy().reshape(A, -1)[:, :n] if n else np.zeros((A, 0), np.int64),
                match=mt[:sizes[5]].cpu().numpy(), match_iou=mi[:sizes[5]].cpu().numpy(),
                status=int(status.item()))


def _device_reduce(t, mc, lc, n_cat, fill=-3):
    import torch
    lib, sizes = _lib.load(), _sizes(t)
    A = len(mc)
    cols = _cells(t) + [_up(t.gt_cat, np.int32), _up(t.gt_flags, np.uint8),
                        _up(t.dt_frame_off, np.int32), _up(t.gt_frame_off, np.int32),
                        _up(mc, np.int32), _up(lc, np.int64)]
    tp = torch.full((n_cat, A), fill, dtype=torch.int64, device=DEV)
    loc = torch.full((n_cat, A), fill, dtype=torch.int64, device=DEV)
    ass = torch.full((n_cat, A, 3), fill, dtype=torch.int64, device=DEV)
    ws = _ws(sizes)
    _lib.check(lib.taoamd_track_hota_reduce(
        *sizes, n_cat, A, *[c.data_ptr() for c in cols], tp.data_ptr(), loc.data_ptr(),
        ass.data_ptr(), ws.data_ptr(), ws.nbytes, _stream()), "taoamd_track_hota_reduce")
    ws.check()
    return tp.cpu().numpy(), loc.cpu().numpy(), ass.cpu().numpy()


def _device_stage(t, alphas, keep=None, n_cat=None, fill=-3):
    n_cat = len(t.cat_ids) if n_cat is None else n_cat
    pot = _device_align(t, keep, fill)
    out = _device_match(t, pot, alphas, keep, fill)
    out["pot"] = pot
    out["tp"], out["loc"], out["ass"] = _device_reduce(t, out["mc"], out["lc"], n_cat, fill)
    return out


def _same_match(got, want):
    assert got["status"] == 0
    assert got["match"].dtype == np.int32 and np.array_equal(got["match"], want["match"])
    assert np.array_equal(got["match_iou"], want["match_iou"])
    assert got["mc"].dtype == np.int32 and np.array_equal(got["mc"], want["mc"])
    assert got["lc"].dtype == np.int64 and np.array_equal(got["lc"], want["lc"])


def _check_groups(got, want):
    """Per frame group the device's pairs are a valid one-to-one set of pairs with
    w > 0 whose weights add up to scipy's optimum on the integer matrix."""
    from scipy.optimize import linear_sum_assignment
    for _, _, gf, dl, W, _, _ in want["groups"]:
        m = got["match"][gf]
        on = np.flatnonzero(m >= 0)
        assert np.isin(m[on], dl).all() and len(set(m[on].tolist())) == len(on)
        j = np.searchsorted(dl, m[on])
        w = W[on, j]
        assert (w > 0).all()
        r, c = linear_sum_assignment(W, maximize=True) if W.size else ([], [])
        assert int(w.sum()) == (int(W[r, c].sum()) if W.size else 0)


# ---------------------------------------------------------------------------
# the seeded table: cells of one, two and three ground truths, a cell of many
# detection tracks and one of many ground truths (both beyond a wavefront),
# empty sides; ground-truth tracks of 63, 64 and 65 frames across a tile edge,
# with holes
# ---------------------------------------------------------------------------
CELLS = [(3, 1), (5, 2), (6, 3), (0, 2), (2, 0), (70, 5), (4, 66), (7, 1), (8, 2), (9, 3)]
LENGTHS = [1, 7, 63, 64, 65, 130]
ALPHAS = ref.HAND_ALPHAS


@pytest.fixture(scope="module")
def seeded():
    """(flat, keep, the restatement with keep, pot of the restatement without)."""
    f = ref.seeded_flat(23, CELLS, LENGTHS)
    keep = (np.random.default_rng(3).random(len(f.dt_cat)) < 0.85).astype(np.uint8)
    want = ref.stage(f, ALPHAS, keep)
    pot_all = ref.align(f, None)
    for v in (want["pot"], want["mc"], want["lc"], want["match"], pot_all):
        v.setflags(write=False)
    return f, keep, want, pot_all


def test_align_on_the_seeded_table(seeded):
    f, keep, want, pot_all = seeded
    # the cases are there
    elig = (np.asarray(f.gt_flags) & 1) == 0
    per_cell = [int(elig[a:b].sum()) for a, b in zip(f.cell_gt_off[:-1], f.cell_gt_off[1:])]
    assert {1, 2, 3} <= set(per_cell) and not elig.all() and not keep.all()
    assert {63, 64, 65} <= set(np.diff(f.gt_frame_off).tolist())
    gaps = np.diff(f.gt_frame_pos)
    assert (gaps[gaps > 0] > 1).any() and (np.diff(f.dt_frame_pos) > 1).any()
    many = sum(len(g[2]) > 1 for g in want["groups"])
    assert many > 100 and (want["pot"] > 0).any() and not np.array_equal(want["pot"], pot_all)
    got = _device_align(f, keep)
    assert got.dtype == np.int64 and np.array_equal(got, want["pot"])
    assert np.array_equal(_device_align(f, None, fill=77), pot_all)


def test_align_on_boxes_that_are_any_double():
    prng = np.random.default_rng(79)
    turn = [0]

    def boxes(n):
        kind = boxpop.KINDS[turn[0] % len(boxpop.KINDS)]
        turn[0] += 1
        return boxpop.box_population(kind, 2 * n, prng)
    f = ref.seeded_flat(94, CELLS[:6], [1, 7, 20, 65], boxes=boxes)
    with np.errstate(all="ignore"):
        every = orclib.bb_iou(np.asarray(f.dt_frame_box)[:2000], np.asarray(f.gt_frame_box)[:500])
    assert np.isnan(every).any()
    want = ref.stage(f, ALPHAS, None)
    assert (want["pot"] > 0).any()
    got = _device_stage(f, ALPHAS, None)
    assert np.array_equal(got["pot"], want["pot"])
    _same_match(got, want)
    for k in ("tp", "loc", "ass"):
        assert np.array_equal(got[k], want[k]), k


def test_all_three_on_the_seeded_table_twice(seeded):
    f, keep, want, _ = seeded
    got = _device_stage(f, ALPHAS, keep)
    _same_match(got, want)
    _check_groups(got, want)
    for k in ("tp", "loc", "ass"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    assert want["tp"].any() and (want["match"] >= 0).any() and (want["match"] < 0).any()
    # determinism: the same bytes from a second run over other junk
    again = _device_stage(f, ALPHAS, keep, fill=77)
    for k in ("pot", "mc", "lc", "match", "match_iou", "tp", "loc", "ass"):
        assert again[k].tobytes() == got[k].tobytes(), k
    # match_iou may be NULL
    lean = _device_match(f, got["pot"], ALPHAS, keep, with_iou=False)
    assert np.array_equal(lean["match"], got["match"]) and (lean["match_iou"] == -3).all()


# ---------------------------------------------------------------------------
# the match alone on given pot tables: one-frame cells, each one frame group
# ---------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 65), (2, 1), (2, 2), (3, 2), (2, 3), (63, 64), (64, 64), (65, 64),
          (3, 256), (2, 257), (257, 2),
          (3, 128), (3, 129), (129, 3)]     # the edge of TH_LDS: the state leaves LDS
FAMILIES = [("dense", 1), ("dense", 19), ("dense", 32), ("sparse", 19), ("equal", 1),
            ("permutation", 32), ("zero_row_and_column", 19), ("w_zero", 32)]


def _family(name, seed):
    rng = np.random.default_rng(seed)
    t = ref.one_frame_table(SHAPES, rng)
    parts = []
    for G, D in SHAPES:
        if name == "dense":
            w = rng.integers(1, ONE + 1, (D, G))
        elif name == "sparse":
            w = rng.integers(1, ONE + 1, (D, G)) * (rng.random((D, G)) < 0.1)
        elif name == "equal":
            w = np.full((D, G), ONE // 2)
        elif name == "permutation":
            w = rng.integers(0, ONE // 64, (D, G))
            n = min(D, G)
            w[rng.permutation(D)[:n], rng.permutation(G)[:n]] = ONE
        elif name == "zero_row_and_column":
            w = rng.integers(1, ONE + 1, (D, G))
            w[:1], w[:, :1] = 0, -5                    # (a negative word reads 0)
        else:
            w = rng.integers(0, 4, (D, G))             # P about 2^-30: w is 0, 1 or 2
        parts.append(np.asarray(w, np.int64).ravel())
    if name == "equal":
        t.dt_frame_box[:, 3] = t.gt_frame_box[:, 3] = 10
    return t, np.concatenate(parts)


@pytest.mark.parametrize("name,n_alpha", FAMILIES)
def test_match_on_given_pot_tables(name, n_alpha):
    t, pot = _family(name, 31 + len(name) + n_alpha)
    alphas = {1: np.array([0.5]), 19: ALPHAS, 32: np.linspace(0.03, 0.99, 32)}[n_alpha]
    want = ref.match(t, pot, alphas)
    # the family holds what it is for
    sizes = {(len(g[2]), len(g[3])) for g in want["groups"]}
    assert sizes == set(SHAPES)
    top = max(int(g[4].max()) for g in want["groups"])
    if name == "w_zero":
        assert top <= 2 and any((g[4] == 0).any() and (g[4] > 0).any() for g in want["groups"])
    elif name == "equal":
        assert all(len(set(g[4].ravel().tolist())) == 1 for g in want["groups"])
    else:
        assert top > ONE // 4
    if name == "zero_row_and_column":
        assert all((g[4][0] == 0).all() and (g[4][:, 0] == 0).all() for g in want["groups"])
    got = _device_match(t, pot, alphas)
    _same_match(got, want)
    _check_groups(got, want)
    matched = sum(len(g[5]) for g in want["groups"])
    assert 0 < int(got["mc"][0].sum()) <= matched
    # mc[a] descends with alpha and lc follows it
    assert (np.diff(got["mc"].astype(np.int64), axis=0) <= 0).all()
    assert ((got["lc"] > 0) == (got["mc"] > 0)).all()


# ---------------------------------------------------------------------------
# the reduction alone on synthetic mc and lc
# ---------------------------------------------------------------------------
def test_reduce_on_synthetic_tables():
    rng = np.random.default_rng(17)
    cells = [(3, 2), (1, 1), (0, 4), (5, 0), (65, 3), (2, 70), (4, 4), (6, 5)]
    n_cat = 3
    cat = [c % n_cat for c in range(len(cells))]
    cat[3], cat[6], cat[7] = 1, -1, n_cat                  # two cells count nowhere
    n_dt, n_gt = sum(d for d, _ in cells), sum(g for _, g in cells)
    flags = (rng.random(n_gt) < 0.25).astype(np.uint8) | (rng.integers(0, 2, n_gt) * 2).astype(np.uint8)
    t = identity_ref.table(cells, cat, flags, np.zeros(n_dt, np.uint8), n_cat, rng)
    t.dt_frame_pos = np.zeros(int(t.dt_frame_off[-1]), np.int32)
    t.gt_frame_pos = np.zeros(int(t.gt_frame_off[-1]), np.int32)
    A, n_iou = 5, int(t.cell_iou_off[-1])
    mc = rng.integers(-3, 12, (A, n_iou)).astype(np.int32)
    mc[rng.random((A, n_iou)) < 0.4] = 0
    lc = rng.integers(-ONE, 9 * ONE, (A, n_iou))
    # m = L_g = F_d: the whole of both tracks matched to each other
    L, F = np.diff(t.gt_frame_off), np.diff(t.dt_frame_off)
    whole = 0
    for c, (D, G) in enumerate(cells):
        for d in range(D):
            for g in range(G):
                lg, fd = L[t.cell_gt_off[c] + g], F[t.cell_dt_off[c] + d]
                if lg == fd and not flags[t.cell_gt_off[c] + g] & 1 and 0 <= cat[c] < n_cat:
                    mc[1, t.cell_iou_off[c] + d * G + g] = lg
                    whole += 1
    assert whole > 3 and (mc < 0).any() and (flags & 1).any()
    want = ref.reduce(t, mc, lc, n_cat)
    assert want[0].any() and want[2].all(2).any()
    got = _device_reduce(t, mc, lc, n_cat)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w)
    again = _device_reduce(t, mc, lc, n_cat, fill=77)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))


# ---------------------------------------------------------------------------
# the hand-written table, the empty sides, the refusals
# ---------------------------------------------------------------------------
def test_all_three_on_the_hand_written_table():
    f, dt_at, gt_at, keep = ref.hand_flat()
    got = _device_stage(f, ALPHAS, keep)
    assert got["status"] == 0
    assert ref.match_by_given(f, dt_at, gt_at, got["match"]) == ref.HAND_MATCH
    iou = [float(got["match_iou"][k]) for g in gt_at
           for k in range(f.gt_frame_off[g], f.gt_frame_off[g + 1])]
    assert iou == ref.HAND_MATCH_IOU
    assert got["tp"].tolist() == ref.HAND_TP and got["ass"][:, :, 0].tolist() == ref.HAND_ASS0
    want = ref.stage(f, ALPHAS, keep)
    assert np.array_equal(got["pot"], want["pot"])
    _same_match(got, want)
    for k in ("tp", "loc", "ass"):
        assert np.array_equal(got[k], want[k]), k
    for alpha, tp in ((0.5, ref.HAND_TP_AT_HALF), (0.5 + 2.0 ** -52, ref.HAND_TP_ABOVE_HALF)):
        assert _device_stage(f, [alpha], keep)["tp"].tolist() == tp


@pytest.mark.parametrize("case", ["no_detection_tracks", "no_ground_truth", "no_cells",
                                  "no_detection_frames", "mixed"])
def test_all_three_on_empty_sides(case):
    import association_ref
    f, _ = association_ref.empty_sides()[case]
    want = ref.stage(f, ALPHAS, None)
    got = _device_stage(f, ALPHAS, None)
    assert np.array_equal(got["pot"], want["pot"])
    _same_match(got, want)
    for k in ("tp", "loc", "ass"):
        assert np.array_equal(got[k], want[k]), k
    if case != "mixed":
        assert not want["tp"].any() and (want["match"] == -1).all()
    else:
        # the long ground truth is followed on the frames the two tracks with boxes have
        assert want["tp"].any() and (want["match"] >= 0).sum() > 10


def test_argument_refusals_launch_nothing():
    import torch
    lib = _lib.load()
    f, _, _, keep = ref.hand_flat()
    sizes = _sizes(f)
    cols = _cells(f) + [_up(f.gt_flags, np.uint8), _up(keep, np.uint8)] + _frames(f)
    n = max(sizes[3], 1)
    pot = torch.full((n,), 5, dtype=torch.int64, device=DEV)
    mc = torch.full((3, n), 77, dtype=torch.int32, device=DEV)
    lc = torch.full((3, n), 77, dtype=torch.int64, device=DEV)
    mt = torch.full((sizes[5],), 77, dtype=torch.int32, device=DEV)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    ws = _ws(sizes)

    def match(alphas, n_alpha=None, nbytes=ws.nbytes):
        a = np.ascontiguousarray(alphas, np.float64)
        return lib.taoamd_track_hota_match(
            *sizes, len(a) if n_alpha is None else n_alpha, a.ctypes.data,
            *[c.data_ptr() for c in cols], pot.data_ptr(), mc.data_ptr(), lc.data_ptr(),
            mt.data_ptr(), None, status.data_ptr(), ws.data_ptr(), nbytes, _stream())
    for bad in ([0.5, 0.5], [0.5, 0.25], [0.25, float("nan"), 0.75], [float("nan")]):
        assert match(bad) == _lib.ERR_ARG, bad
    assert match(np.linspace(0.1, 0.9, 33)) == _lib.ERR_ARG
    assert match([0.5], n_alpha=0) == _lib.ERR_ARG
    assert match([0.25, 0.5, 0.75], nbytes=ws.nbytes - 1) == 4
    assert lib.taoamd_track_hota_align(
        *sizes, *[c.data_ptr() for c in cols], pot.data_ptr(), ws.data_ptr(), ws.nbytes - 1,
        _stream()) == 4
    ws.check()
    assert int(status.item()) == 77 and bool((mc == 77).all()) and bool((mt == 77).all())
    assert bool((pot == 5).all()) and bool((lc == 77).all())
    assert match([0.25, 0.5, 0.75]) == _lib.OK
    ws.check()
    assert int(status.item()) == 0 and not bool((mt == 77).any())


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
    from tao_amodal_amd.evaluation.tao_amodal import followers
    ev = _tao(name)
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.hota()
    ev.evaluate()
    ev.accumulate()
    before = {k: ev.eval[k].copy() for k in ("precision", "recall")}
    flat = ev._run.flat
    ident = identity_ref.identity(flat, 0.5)
    keep = ident["kept"].astype(np.uint8)
    want = ref.stage(flat, ref.DEFAULT_ALPHAS - np.finfo(float).eps, keep)
    cats = np.asarray(flat.cat_ids).tolist()
    pos = [cats.index(int(c)) for c in ev.params.cat_ids]
    got = ev.hota()
    K, A = len(ev.params.cat_ids), 19
    assert "frames" not in got and got["frame_thr"] == 0.5
    assert np.array_equal(got["alphas"], ref.DEFAULT_ALPHAS)
    counts = ident["cat_counts"][pos][:, :4]
    assert np.array_equal(got["cat_counts"], counts) and got["cat_counts"].dtype == np.int64
    for k in ("tp", "loc", "ass"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k][pos]), k
    assert got["tp"].shape == (K, A) and got["ass"].shape == (K, A, 3) and got["tp"].any()
    assert np.array_equal(got["fn"], counts[:, 1:2] - got["tp"]) and (got["fn"] >= 0).all()
    assert np.array_equal(got["fp"], counts[:, 3:4] - got["tp"]) and (got["fp"] >= 0).all()
    r = ref.ratios(want["tp"][pos], want["loc"][pos], want["ass"][pos], counts[:, 1:2],
                   counts[:, 3:4])
    has = (counts[:, 1] + counts[:, 3]) > 0
    for k in ref.RATIOS:
        w = np.where(has[:, None], r[k], np.nan)
        assert got[k].dtype == np.float64 and np.array_equal(got[k], w, equal_nan=True), k
    tot = got["total"]
    assert np.array_equal(tot["tp"], want["tp"].sum(0)) and tot["gt_frames"] == counts[:, 1].sum()
    rt = ref.ratios(tot["tp"], want["loc"].sum(0), want["ass"].sum(0), tot["gt_frames"],
                    tot["dt_frames"])
    for k in ref.RATIOS:
        assert np.array_equal(tot[k], rt[k]), k
    assert tot["HOTA"] == float(rt["hota"].mean()) and 0 < tot["HOTA"] <= 1
    assert tot["HOTALocA(0)"] == float(rt["hota"][0] * rt["loca"][0])
    assert got["mean"]["HOTA"] == float(r["hota"].mean(1)[has].mean())
    # a one-to-one frame assignment matches no more frames than are covered
    assert tot["tp"][0] <= ev.association(frame_thr=0.05)["cat_counts"][:, 2].sum()
    assert ev.hota()["tp"] is got["tp"]                                        # cached
    full = ev.hota(per_frame=True)
    assert full["tp"] is got["tp"]
    gid, img, did, s = full["frames"]
    foff, cell, want_img = followers._gt_frame_tables(flat)
    g_of = np.repeat(np.arange(len(foff) - 1), np.diff(foff))
    assert np.array_equal(gid, np.asarray(flat.gt_id)[g_of]) and np.array_equal(img, want_img)
    assert np.array_equal(did, followers._follower_ids(flat, cell, want["match"]))
    assert np.array_equal(s, want["match_iou"]) and (did >= 0).sum() == (s > 0).sum() > 0
    lines = ev.hota_lines()
    assert len(lines) == 4 and "HOTA" in lines[1] and lines[2].split()[0] == "total"
    # other alphas: another table under another key
    one = ev.hota(alphas=[0.5, 0.75])
    w2 = ref.stage(flat, np.array([0.5, 0.75]) - np.finfo(float).eps, keep)
    assert one["tp"].shape == (K, 2) and np.array_equal(one["tp"], w2["tp"][pos])
    assert np.array_equal(one["ass"], w2["ass"][pos]) and len(ev._hota) == 2
    # the identity was computed on the way and is what identity() returns
    assert np.array_equal(ev.identity()["cat_counts"], ident["cat_counts"][pos])
    for k, v in before.items():
        assert np.array_equal(ev.eval[k], v, equal_nan=True), k


def test_class_api_refusals():
    ev = _tao("f1")
    ev.evaluate()
    for bad in ([0.0, 0.5], [0.5, 0.5], [0.5, 1.5], np.linspace(0.01, 0.99, 33)):
        with pytest.raises(ValueError, match="alphas"):
            ev.hota(bad)
    with pytest.raises(ValueError, match="frame_thr"):
        ev.hota(frame_thr=0.0)
    from tao_amodal_amd import engine
    with pytest.raises(_lib.TaoAmdError, match="alphas"):
        engine.stage_track_hota(ev._run.dp, ev._run.ws, np.linspace(0.01, 0.99, 33), 0.5)
    pooled = _tao("f1")
    pooled.params.use_cats = 0
    pooled.evaluate()
    with pytest.raises(NotImplementedError, match="use_cats = 0"):
        pooled.hota()
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval
    segm = TaoEval(Tao(path("f6", "gt.json")), path("f6", "pred_rle.json"), iou_type="segm")
    segm.evaluate()
    with pytest.raises(NotImplementedError, match="iou_type='segm'"):
        segm.hota()
    with pytest.raises(_lib.TaoAmdError, match="on boxes"):
        engine.stage_track_hota(segm._run.dp, segm._run.ws, [0.5], 0.5)
    from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
    assert not hasattr(LVISEval, "hota")                    # the track level's alone
    image = ev._run
    kind = image.flat.kind
    image.flat.kind = "lvis"
    with pytest.raises(NotImplementedError, match="track level"):
        ev.hota()
    image.flat.kind = kind
    # a multi-GPU run: its evaluator refuses, and nothing is cached
    from tao_amodal_amd.evaluation._dist import DistRun
    ev._run = DistRun.__new__(DistRun)
    with pytest.raises(NotImplementedError, match=r"hota\(\) in a multi-GPU run"):
        ev.hota()
    with pytest.raises(NotImplementedError, match=r"hota\(\) in a multi-GPU run"):
        ev.hota_lines()
    assert ev._hota == {}
