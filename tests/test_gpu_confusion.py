"""-m gpu: the confusion table (taoamd_confusion_count, taoamd_confusion_fill,
engine.stage_confusion, LVISEval.confusion, TaoEval.confusion) against the numpy
restatement of tests/confusion_ref.py.  Every value is an integer and every
entry has one place: every comparison is exact."""
import json
import os
import sys

import numpy as np
import pytest

import confusion_ref as ref
import error_impact_ref as imp
import error_types_ref as et
import orclib
import track_error_impact_ref as timp
import wsguard
from goldenio import GOLDEN as GOLDEN_DIR, load_inputs, input_paths
from tao_amodal_amd import _lib

sys.path.insert(0, GOLDEN_DIR)
from constants_cases import cases, edit  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = _lib.CONFUSION_TILE
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
JUNK = -5            # what the output arrays hold before a call
GUARD = 3            # entries behind `cap` that no call may touch
CLS, BOTH, TP = et.CLS, et.BOTH, et.TP


def _up(a, dtype, shape=None):
    import torch
    a = np.array(a, dtype=dtype)           # (a copy: a fixture's tables are read-only)
    if shape is not None:
        a = a.reshape(shape)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], dtype=dtype)
    return torch.from_numpy(a).to(DEV)


def _device(n_cat, n_rng, cat_off, score, dt_cat, dt_type, link_other, gt_cat, held, cap=None,
            status=False, ws_bytes=None, misalign=False):
    """count, then fill, on bare tables.  The workspace is exactly the size
    reported, behind a guard band, and the same buffer for both calls; the
    outputs start as junk, with GUARD entries behind `cap` (default: the
    total).  Returns (ent_off, ent_gt_cat, ent_counts, total), the two entry
    arrays with their guard entries."""
    import torch
    lib = _lib.load()
    n_dt, n_gt = len(dt_cat), len(gt_cat)
    cols = [_up(cat_off, np.int32), _up(score, np.float64), _up(dt_cat, np.int32),
            _up(dt_type, np.uint8, (n_dt, n_rng)), _up(link_other, np.int32, (n_dt, n_rng)),
            _up(gt_cat, np.int32), _up(held, np.uint8, (n_rng, n_gt))]
    off = torch.full((n_rng * n_cat + 1,), -77, dtype=torch.int64, device=DEV)
    need = lib.taoamd_confusion_workspace(n_dt, n_gt, n_cat, n_rng)
    ws = wsguard.Guarded(need if ws_bytes is None else ws_bytes, DEV)
    s = torch.cuda.current_stream().cuda_stream
    head = [n_dt, n_gt, n_cat, n_rng] + [c.data_ptr() for c in cols]
    st = lib.taoamd_confusion_count(*head, off.data_ptr(), ws.data_ptr(), ws.nbytes, s)
    if status and st:
        torch.cuda.synchronize()
        return st
    _lib.check(st, "taoamd_confusion_count")
    total = int(off[-1].item())
    assert total >= 0
    cap = total if cap is None else cap
    ent_cat = torch.full((cap + GUARD,), JUNK, dtype=torch.int32, device=DEV)
    ent_n = torch.full((cap + GUARD + 1, 4), JUNK, dtype=torch.int32, device=DEV)
    counts = ent_n.view(-1)[1:].view(-1)[:4 * (cap + GUARD)].view(-1, 4) if misalign \
        else ent_n[:cap + GUARD]
    st = lib.taoamd_confusion_fill(*head, off.data_ptr(), cap, ent_cat.data_ptr(),
                                   counts.data_ptr(), ws.data_ptr(), ws.nbytes, s)
    if status:
        torch.cuda.synchronize()
        return st
    _lib.check(st, "taoamd_confusion_fill")
    ws.check()
    return off.cpu().numpy(), ent_cat.cpu().numpy(), counts.cpu().numpy(), total


def _same(t, cap=None):
    """The device on the tables `t` == the restatement; nothing behind the
    entries is touched.  Returns the pairs."""
    pairs = ref.confusion_tables(**t)
    want_off, want_cat, want_n = ref.csr(pairs, t["n_cat"], t["n_rng"])
    off, cat, n, total = _device(cap=cap, **t)
    assert np.array_equal(off, want_off) and total == len(want_cat)
    cap = total if cap is None else cap
    # the (a, c) rows that end at or below cap are written, whole; nothing else is
    written = np.zeros(cap + GUARD, bool)
    for row in range(len(off) - 1):
        if off[row + 1] <= cap:
            written[off[row]:off[row + 1]] = True
    k = min(cap, total)
    assert np.array_equal(cat[:k][written[:k]], want_cat[:k][written[:k]])
    assert np.array_equal(n[:k][written[:k]], want_n[:k][written[:k]])
    assert (cat[~written] == JUNK).all() and (n[~written] == JUNK).all()
    return pairs


def _tables(n_cat, n_rng, sizes, gt_cat, seed, p_held=0.4, types=(0, 1, 2, 3, 4, 4, 4, 5, 5, 6)):
    """Seeded bare tables: `sizes` = {category: rows}; every row links a random
    ground truth (a few none) in every range."""
    rng = np.random.default_rng(seed)
    dt_cat = np.repeat(np.array(sorted(sizes), np.int64), [sizes[c] for c in sorted(sizes)])
    n_dt, n_gt = len(dt_cat), len(gt_cat)
    link = rng.integers(0, n_gt, (n_dt, n_rng))
    link[rng.random((n_dt, n_rng)) < 0.05] = -1
    return dict(n_cat=n_cat, n_rng=n_rng, cat_off=ref.segments(dt_cat, n_cat),
                score=rng.choice([0.0, 0.25, 0.5, 0.5, 0.75, 1.0, NAN], n_dt), dt_cat=dt_cat,
                dt_type=rng.choice(types, (n_dt, n_rng)).astype(np.uint8), link_other=link,
                gt_cat=np.asarray(gt_cat, np.int64), held=rng.random((n_rng, n_gt)) < p_held)


def _totals(pairs):
    return [sum(n[i] for n in pairs.values()) for i in range(4)]


# ---------------------------------------------------------------------------
# the category axis: around the LDS tile
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_cat", [2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_categories_around_the_tile(n_cat):
    """A few hundred rows in the first, a middle and the last category; their
    links hit the first and the last category of every tile and both sides of
    every tile edge."""
    edges = sorted({c for c in (0, 1, TILE - 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE,
                                n_cat - 2, n_cat - 1) if 0 <= c < n_cat})
    gt_cat = np.repeat(edges, 3)
    sizes = {0: 120, n_cat // 2: 70, n_cat - 1: 130}
    t = _tables(n_cat, 2, sizes, gt_cat, seed=n_cat)
    pairs = _same(t)
    tot = _totals(pairs)
    assert tot[0] > tot[2] > tot[3] > 0 and tot[1] > 0
    assert {c2 for _, _, c2 in pairs} == set(edges)
    assert {c for _, c, _ in pairs} == set(sizes)


def test_one_category_has_no_entries():
    """n_cat = 1: a link names a ground truth of the row's own category, which
    the breakdown never produces; without links there is no entry."""
    t = _tables(1, 2, {0: 100}, [0, 0, 0], seed=1)
    t["link_other"][:] = -1
    off, cat, n, total = _device(**t)
    assert total == 0 and (off == 0).all() and (cat == JUNK).all() and (n == JUNK).all()


# ---------------------------------------------------------------------------
# the segments of the predicted categories
# ---------------------------------------------------------------------------
SIZES = [1, 0, 63, 64, 65, 255, 256, 257, 1025, 2]


def test_segment_lengths_around_the_wavefront_and_the_workgroup():
    """An empty category, the first and the last category non-empty, a cat_off
    that runs past the table (clamped)."""
    K = len(SIZES)
    gt_cat = np.repeat(np.arange(K), 2)
    t = _tables(K, 6, dict(enumerate(SIZES)), gt_cat, seed=5)
    t["cat_off"] = t["cat_off"].copy()
    t["cat_off"][-1] += 1000
    pairs = _same(t)
    assert {c for _, c, _ in pairs} == {c for c in range(K) if SIZES[c]}
    assert {a for a, _, _ in pairs} == set(range(6))
    # every row of the longest category was counted
    long = [n for (a, c, _), n in pairs.items() if c == 8 and a == 0]
    assert sum(n[0] + n[1] for n in long) == int(
        (np.isin(t["dt_type"][t["dt_cat"] == 8, 0], (CLS, BOTH))
         & (t["link_other"][t["dt_cat"] == 8, 0] >= 0)).sum())


# ---------------------------------------------------------------------------
# ranges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_rng", [1, 6, 8, 20])
def test_ranges(n_rng):
    t = _tables(4, n_rng, {0: 90, 1: 70, 3: 80}, [0, 1, 1, 2, 3, 3], seed=40 + n_rng)
    # row 0: CLS in the last range, BOTH in range 1 (where there is one), TP in the rest
    t["dt_type"][0] = TP
    t["dt_type"][0, n_rng - 1] = CLS
    if n_rng > 1:
        t["dt_type"][0, 1] = BOTH
    t["link_other"][0] = 3                    # of category 2, which no other row links
    t["link_other"][1:][t["link_other"][1:] == 3] = 4
    t["held"][:, 3] = False
    pairs = _same(t)
    want = {(n_rng - 1, 0, 2): [1, 0, 1, 1]}
    if n_rng > 1:
        want[(1, 0, 2)] = [0, 1, 0, 0]
    assert {k: v for k, v in pairs.items() if k[2] == 2} == want
    assert {a for a, _, _ in pairs} == set(range(n_rng))


# ---------------------------------------------------------------------------
# rows that are skipped
# ---------------------------------------------------------------------------
def test_rows_outside_the_tables_are_skipped():
    n_gt, K = 4, 3
    big = 2 ** 31 - 1
    #        row: 0    1     2    3    4     5    6    7    8    9    10   11
    dt_cat = [0,   0,    0,   0,   0,    0,   0,   -1,  1,   1,   3,   1]
    ty = [CLS, CLS,  CLS, CLS, BOTH, CLS, 7,   CLS, 255, CLS, CLS, BOTH]
    link = [1,   -1,   n_gt, big, 2,   3,   1,   1,   0,   0,   0,   0]
    gt_cat = [0, 1, -1, K]            # gt 2 and gt 3: categories outside the table
    # segments: category 0 = rows 0-7 (row 7 carries -1), category 1 = rows 8-10
    # (row 10 carries 3 = n_cat), category 2 = row 11 (it carries 1)
    t = dict(n_cat=K, n_rng=1, cat_off=[0, 8, 11, 12], score=np.linspace(1, 0, 12),
             dt_cat=dt_cat, dt_type=ty, link_other=link, gt_cat=gt_cat, held=[[0, 0, 0, 0]])
    pairs = _same(t)
    # row 0 -> (0, 1); row 9 -> (1, 0); everything else is skipped
    assert pairs == {(0, 0, 1): [1, 0, 1, 1], (0, 1, 0): [1, 0, 1, 1]}


# ---------------------------------------------------------------------------
# winners
# ---------------------------------------------------------------------------
# (score of the contender of category 1, in the lower row; of category 2; the winner's category)
DUELS = [(0.5, 0.5, 1), (-0.0, 0.0, 1), (0.0, -0.0, 1), (1e308, INF, 2), (-INF, NAN, 1),
         (NAN, -INF, 2), (0.0, 5e-324, 2), (-5e-324, -0.0, 2), (NAN, NAN, 1), (-INF, -1e308, 2),
         (2.5, 1.5, 1)]


@pytest.mark.parametrize("held_last", [False, True])
def test_winner_rule_between_two_predicted_categories(held_last):
    """Ground truth i, alone in category 3 + i, is linked by one CLS row of
    category 1 and one of category 2: exactly one of the two pairs gets the
    `adopted`.  Equal scores and -0.0 against 0.0 go to the lower row; +-inf and
    subnormals compare as numbers; a NaN loses to every number; between two NaNs
    the lower row wins.  A held ground truth is neither unheld nor adopted."""
    n = len(DUELS)
    K = 3 + n
    t = dict(n_cat=K, n_rng=1, cat_off=[0, 0, n, 2 * n] + [2 * n] * n,
             score=[d[0] for d in DUELS] + [d[1] for d in DUELS],
             dt_cat=[1] * n + [2] * n, dt_type=[CLS] * (2 * n), link_other=list(range(n)) * 2,
             gt_cat=list(range(3, K)), held=[[0] * (n - 1) + [int(held_last)]])
    pairs = _same(t)
    want = {}
    for i, (_, _, w) in enumerate(DUELS):
        held = held_last and i == n - 1
        for c in (1, 2):
            want[(0, c, 3 + i)] = [1, 0, int(not held), int(c == w and not held)]
    assert pairs == want


# ---------------------------------------------------------------------------
# contention, and sizes of nothing
# ---------------------------------------------------------------------------
def test_seventy_thousand_rows_on_one_counter():
    rng = np.random.default_rng(9)
    n = 70000
    t = dict(n_cat=2, n_rng=1, cat_off=[0, n, n], score=rng.integers(0, 20, n) / 20.0,
             dt_cat=np.zeros(n, np.int64), dt_type=np.full(n, CLS, np.uint8),
             link_other=rng.integers(0, 7, n), gt_cat=[1] * 7, held=[[0, 1, 0, 0, 1, 0, 0]])
    pairs = _same(t)
    (key, counts), = pairs.items()
    assert key == (0, 0, 1) and counts[0] == n and counts[3] == 5 and 0 < counts[2] < n


def test_no_rows_and_no_ground_truths():
    t = _tables(3, 6, {}, [0, 1, 2], seed=3)
    off, cat, n, total = _device(**t)
    assert total == 0 and (off == 0).all() and len(off) == 19
    t = _tables(3, 6, {0: 70, 2: 5}, [0], seed=3)
    t.update(gt_cat=np.zeros(0, np.int64), held=np.zeros((6, 0), bool))
    t["link_other"][:] = -1
    off, cat, n, total = _device(**t)
    assert total == 0 and (off == 0).all() and (cat == JUNK).all()
    assert ref.confusion_tables(**t) == {}


# ---------------------------------------------------------------------------
# the cap protocol, repeatability, the workspace
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    t = _tables(6, 6, {0: 130, 2: 300, 3: 64, 5: 9}, np.repeat(np.arange(6), 2), seed=77)
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def test_cap_protocol(small):
    total = len(ref.confusion_tables(**small))
    assert total > 20
    _same(small, cap=total)
    _same(small, cap=total - 1)          # the last (a, c) row is left out, whole
    _same(small, cap=total // 2)
    _same(small, cap=0)
    _same(small, cap=total + 2)


def test_two_runs_are_byte_identical(small):
    a, b = _device(**small), _device(**small)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()


def test_workspace_base_moved_by_8_bytes(small, monkeypatch):
    monkeypatch.setattr(wsguard, "SHIFT", 8)
    _same(small)


def test_abi_error_paths(small):
    lib = _lib.load()
    need = lib.taoamd_confusion_workspace(len(small["dt_cat"]), len(small["gt_cat"]), 6, 6)
    assert _device(status=True, **small) == 0
    assert _device(status=True, ws_bytes=need - 1, **small) == 4
    assert _device(status=True, cap=-1, **small) == 2
    assert _device(status=True, misalign=True, **small) == 2     # ent_counts off 16 bytes


# ---------------------------------------------------------------------------
# the class API, end to end
# ---------------------------------------------------------------------------
def _evaluator(level, name, relabel, tmp_path):
    gt_path, dt_path = input_paths(name, tmp_path)
    if relabel:
        gtj, predj = load_inputs(name)
        dt_path = os.path.join(str(tmp_path), "relabelled.json")
        with open(dt_path, "w") as fh:
            json.dump(ref.relabelled(gtj, predj), fh)
    if level == "lvis":
        from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
        return LVISEval(gt_path, dt_path, "bbox")
    from tao_amodal_amd import flatten
    from tao_amodal_amd.columns import DTColumns
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval, TaoResults
    dt = DTColumns.from_json(dt_path)
    dt.track_id, _ = flatten.make_track_ids_unique(dt)
    gt = Tao(gt_path)
    return TaoEval(gt, TaoResults(gt, dt))


def _restated(ev, iou_thr, bg_thr):
    """The restatement on the evaluator's own tables: IoU matrix, match indices
    and range masks of a detail-mode pass under the evaluator's constants, types
    and links by the reference functions; the kernels' range slots put in the
    caller's order, the categories in the order of params.cat_ids.  Returns
    (rng, dt_cat ids, gt_cat ids, counts) as confusion() returns them."""
    import torch
    from tao_amodal_amd import engine
    from tao_amodal_amd.evaluation._core import applied
    run = ev._run
    c, f = run.constants, run.flat
    track = f.kind == "tao"
    ws = engine.Workspace(run.dp, detail=True)
    with applied(c):
        engine.run_guarded(run.dp, ws, f, upto="match")
        torch.cuda.synchronize()
    n_dt, n_gt = run.dp.n_dt, run.dp.n_gt
    mg = ws.match_gt[:n_dt].cpu().numpy()
    gt_rng = ws.gt_rng[:n_gt].cpu().numpy().view(np.uint32)
    thrs = orclib.thresholds()[0] if c is None else c.thr_blocks[0][1]
    i = int(np.where(iou_thr == np.asarray(ev.params.iou_thrs))[0][0])
    slot = i if c is None else int(np.where(c.thr_blocks[0][0] == i)[0][0])
    assert thrs[slot] == iou_thr
    P = ev.params
    if track:
        dt_rng = ws.dt_rng[:n_dt].cpu().numpy().view(np.uint32)
        iou = ws.iou[:run.dp.n_iou].cpu().numpy()
        want = timp.error_impact(f, iou, mg, gt_rng, dt_rng, thrs, slot, bg_thr)
        A, T = len(P.area_rng), len(P.time_rng)
        ks = [(a if a < A - 1 else 4) * 4 + t for a in range(A) for t in range(T)]
        n_rng = 20
    else:
        want = imp.error_impact(f, mg, gt_rng, thrs, slot, bg_thr)
        ks = list(range(len(P.visibility_rng) - 1)) + [5]
        n_rng = 6
    pairs = ref.of_impact(f, want, n_rng)
    to = {k: a for a, k in enumerate(ks)}
    cats = np.asarray(f.cat_ids).tolist()
    place = {cats.index(int(k)): j for j, k in enumerate(P.cat_ids)}
    rows = sorted((to[a], place[k], place[k2], n) for (a, k, k2), n in pairs.items()
                  if a in to and k in place and k2 in place)
    ids = np.asarray(P.cat_ids, dtype=np.int64)
    return (np.array([r[0] for r in rows], np.int32),
            ids[np.array([r[1] for r in rows], np.int64)],
            ids[np.array([r[2] for r in rows], np.int64)],
            np.array([r[3] for r in rows], np.int64).reshape(-1, 4))


def _check_class_api(ev, iou_thr, bg_thr, monkeypatch, whole=True):
    """confusion() == the restatement; with `whole` (every category, the
    reference's constants) the three invariants against error_types() and
    error_impact() of the same evaluator.  Returns the result."""
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.confusion(iou_thr, bg_thr)
    ev.evaluate()
    rng, dt_cat, gt_cat, counts = _restated(ev, iou_thr, bg_thr)
    calls = []
    table = ev._run.confusion_table
    monkeypatch.setattr(ev._run, "confusion_table", lambda *a: calls.append(a) or table(*a))
    got = ev.confusion(iou_thr, bg_thr)
    types = ev.error_types(iou_thr, bg_thr)
    assert got["columns"] == list(ref.COLUMNS) and got["rng_lbl"] == types["rng_lbl"]
    assert got["rng"].dtype == np.int32 and got["counts"].dtype == np.int64
    assert np.array_equal(got["rng"], rng)
    assert np.array_equal(got["dt_cat"], dt_cat) and np.array_equal(got["gt_cat"], gt_cat)
    assert np.array_equal(got["counts"], counts)
    assert ev.confusion(iou_thr, bg_thr)["counts"] is got["counts"] and len(calls) == 1
    n_rng, K = types["dt_counts"].shape[:2]
    ids = list(ev.params.cat_ids)
    # the dense view: its sums are the sparse counts, its diagonal is empty
    for a in sorted(set(got["rng"].tolist()))[:3]:
        for j, col in enumerate(got["columns"]):
            m = ev.confusion_matrix(iou_thr, bg_thr, a, col)
            assert m.shape == (K, K) and m.sum() == got["counts"][got["rng"] == a, j].sum()
            assert (np.diag(m) == 0).all()
    lines = ev.confusion_lines(iou_thr, bg_thr, top=3)
    assert len(lines) == 2 + min(3, int((got["rng"] == 0).sum()))
    assert lines[0].startswith(ev._level + " confusion @[ IoU=%0.2f" % iou_thr)
    assert (got["counts"][:, 3] <= got["counts"][:, 2]).all()
    assert (got["counts"][:, 2] <= got["counts"][:, 0]).all()
    assert (got["counts"][:, 0] + got["counts"][:, 1] > 0).all()
    if whole:
        cls = np.zeros((n_rng, K), np.int64)
        both = np.zeros((n_rng, K), np.int64)
        into = np.zeros((n_rng, K), np.int64)
        at = np.array([ids.index(c) for c in got["dt_cat"].tolist()], np.int64)
        to = np.array([ids.index(c) for c in got["gt_cat"].tolist()], np.int64)
        np.add.at(cls, (got["rng"], at), got["counts"][:, 0])
        np.add.at(both, (got["rng"], at), got["counts"][:, 1])
        np.add.at(into, (got["rng"], to), got["counts"][:, 3])
        assert np.array_equal(cls, types["dt_counts"][:, :, CLS])
        assert np.array_equal(both, types["dt_counts"][:, :, BOTH])
        # the impact's CLS fix adopts into (c', a) exactly where `adopted` says so:
        # adopted rows are true positives, so the recall the category reaches
        # grows with them and with nothing else of that fix.  Up to 50
        # evaluated ground truths every count is the crossing of a threshold.
        p = ev.error_impact(iou_thr, bg_thr)["precision"]
        reached = (p > 0).sum(1)                      # [9, K, n_rng]
        ng = types["gt_counts"][:, :, 0]
        ok = (ng > 0) & (ng <= 50)
        assert ok.any()
        grew = (reached[imp.F_CLS] > reached[imp.BASE]).T
        assert np.array_equal(grew[ok], into[ok] > 0)
        assert (reached[imp.F_CLS] >= reached[imp.BASE]).all()
    # a new evaluate() forgets the table
    ev.evaluate()
    assert ev._confusion == {}
    return got


# (level, fixture, relabelled): where the comparison must be of something.  The
# recorded fixtures hold few classification errors -- CLS rows on the image side
# of f1 alone --, so each is also run with every third track relabelled
RICH = {("lvis", "f1", False), ("lvis", "f1", True), ("lvis", "f4", True), ("lvis", "f10", True),
        ("tao", "f1", True), ("tao", "f10", True)}


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("name", ["f1", "f4", "f10"])
@pytest.mark.parametrize("level", ["lvis", "tao"])
def test_class_api_on_the_fixtures(level, name, relabel, tmp_path, monkeypatch):
    ev = _evaluator(level, name, relabel, tmp_path)
    got = _check_class_api(ev, 0.5, 0.1, monkeypatch)
    if (level, name, relabel) in RICH:
        assert got["counts"][:, 0].sum() > 0 and got["counts"][:, 3].sum() > 0


@pytest.mark.parametrize("level,name", [("lvis", "f1"), ("lvis", "f10"), ("tao", "f10")])
def test_class_api_at_another_threshold(level, name, tmp_path, monkeypatch):
    ev = _evaluator(level, name, True, tmp_path)
    got = _check_class_api(ev, ev.params.iou_thrs[5], 0.3, monkeypatch)
    assert got["counts"][:, 0].sum() > 0 and got["counts"][:, 3].sum() > 0


@pytest.mark.parametrize("level", ["lvis", "tao"])
def test_class_api_under_edited_range_constants(level, tmp_path, monkeypatch):
    """Three visibility ranges (kernel slots 0, 1 and the out-of-frame one);
    three area ranges x two durations (slots 0, 1 and the occlusion one; 0, 1)."""
    ev = _evaluator(level, "f1", True, tmp_path)
    edit(ev.params, cases()["ranges3"], level)
    got = _check_class_api(ev, 0.5, 0.1, monkeypatch, whole=False)
    n_rng = 3 if level == "lvis" else 6
    types = ev.error_types(0.5, 0.1)
    assert types["dt_counts"].shape[0] == n_rng and got["rng"].max() < n_rng
    assert got["counts"][:, 0].sum() > 0
    for a in range(n_rng):
        assert got["counts"][got["rng"] == a, 0].sum() == types["dt_counts"][a, :, CLS].sum()


@pytest.mark.parametrize("level", ["lvis", "tao"])
def test_class_api_on_a_params_subset(level, tmp_path, monkeypatch):
    ev = _evaluator(level, "f1", True, tmp_path)
    ids = [ev.params.cat_ids[i] for i in (4, 0, 2, 1)]
    ev.params.cat_ids = list(ids)
    got = _check_class_api(ev, 0.5, 0.1, monkeypatch, whole=False)
    assert set(got["dt_cat"].tolist()) | set(got["gt_cat"].tolist()) <= set(ids)
    assert len(got["rng"]) > 0
    key = [(r, ids.index(d), ids.index(g)) for r, d, g in
           zip(got["rng"].tolist(), got["dt_cat"].tolist(), got["gt_cat"].tolist())]
    assert key == sorted(key) and len(set(key)) == len(key)
    assert ev.confusion_matrix(0.5, 0.1).shape == (4, 4)


def test_class_api_refusals(tmp_path):
    from goldenio import path
    from tao_amodal_amd import engine
    from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
    ev = _evaluator("lvis", "f1", False, tmp_path)
    ev.evaluate()
    with pytest.raises(ValueError, match="not one of params.iou_thrs"):
        ev.confusion(0.55000001)
    with pytest.raises(ValueError, match="bg_thr"):
        ev.confusion(0.5, 0.5)
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_confusion(ev._run.dp, ev._run.ws, 10, 0.1)
    wide = _evaluator("lvis", "f1", False, tmp_path)
    edit(wide.params, cases()["ranges8"], "lvis")
    wide.evaluate()
    with pytest.raises(NotImplementedError, match="one block of ranges"):
        wide.confusion(0.5)
    pooled = _evaluator("tao", "f1", False, tmp_path)
    pooled.params.use_cats = 0
    pooled.evaluate()
    with pytest.raises(NotImplementedError, match="use_cats = 0"):
        pooled.confusion(0.5)
    segm = LVISEval(path("f6", "gt.json"), path("f6", "pred_rle.json"), "segm")
    segm.evaluate()
    with pytest.raises(NotImplementedError, match="iou_type='segm'"):
        segm.confusion(0.5)
