"""-m gpu: the error impact (taoamd_error_types_links, taoamd_error_impact,
engine.stage_error_impact, LVISEval.error_impact) against the numpy restatement
of tests/error_impact_ref.py.  The restatement sweeps every variant's list with
the reference's own arithmetic: every comparison is exact."""
import json
import sys

import numpy as np
import pytest

import error_impact_ref as ref
import error_types_ref as et
import orclib
import test_error_impact_host as hand
import wsguard
from goldenio import GOLDEN as GOLDEN_DIR, input_paths, path
from tao_amodal_amd import _lib

sys.path.insert(0, GOLDEN_DIR)
from constants_cases import cases, edit  # noqa: E402

pytestmark = pytest.mark.gpu

N_THR, N_REC = _lib.N_THR, _lib.N_REC
TILE = _lib.ERROR_TYPES_TILE
CHUNK = _lib.ERROR_IMPACT_CHUNK
DEV = "cuda:0"
NAN = float("nan")
EVENTS = ("winner", "lost_to_held", "lost_to_better", "adopted", "unlinked_missed")


def _up(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], dtype=dtype)
    return torch.from_numpy(a).to(DEV)


def _device_match(f, gt_rng, n_rng):
    """match_gt[n_dt, n_rng * 10] of taoamd_match itself."""
    import torch
    lib = _lib.load()
    n_dt = int(f.cell_dt_off[-1])
    nw = (n_rng * N_THR + 63) // 64
    d_off, g_off = _up(f.cell_dt_off, np.int32), _up(f.cell_gt_off, np.int32)
    dbox, gbox = _up(f.dt_box, np.float64), _up(f.gt_box, np.float64)
    rng, gfl, dfl = _up(gt_rng, np.uint32).view(torch.int32), _up(f.gt_flags, np.uint8), \
        _up(f.dt_flags, np.uint8)
    matched = torch.zeros((max(n_dt, 1), nw), dtype=torch.int64, device=DEV)
    ignored = torch.zeros_like(matched)
    mg = torch.full((max(n_dt, 1), n_rng * N_THR), -7, dtype=torch.int32, device=DEV)
    max_g = int(np.diff(f.cell_gt_off).max()) if f.n_cells else 0
    _lib.check(lib.taoamd_match(
        f.n_cells, d_off.data_ptr(), g_off.data_ptr(), None, max_g, dbox.data_ptr(),
        gbox.data_ptr(), None, n_rng, rng.data_ptr(), None, gfl.data_ptr(), dfl.data_ptr(),
        None, 0, matched.data_ptr(), ignored.data_ptr(), mg.data_ptr(), None, None, None,
        None, 0, None, 0, torch.cuda.current_stream().cuda_stream), "taoamd_match")
    torch.cuda.synchronize()
    return mg[:n_dt].cpu().numpy()


def _device_types(f, mg, gt_rng, n_rng, slot, tb, links=True, status=False, ws_bytes=None,
                  drop=None):
    """taoamd_error_types_links (or, links=False, taoamd_error_types) on a Flat;
    the workspace is exactly the size reported, behind a guard band."""
    import torch
    lib = _lib.load()
    n_dt, n_gt = int(f.cell_dt_off[-1]), int(f.cell_gt_off[-1])
    n_img, K = len(f.img_ids), len(f.cat_ids)
    d_img, g_img = et.units(f)

    def csr(unit):
        off = np.zeros(n_img + 1, np.int32)
        np.cumsum(np.bincount(unit, minlength=n_img), out=off[1:])
        return _up(off, np.int32), _up(np.argsort(unit, kind="stable"), np.int32)
    g_off, g_rows = csr(g_img)
    d_off, d_rows = csr(d_img)
    d_cell = np.repeat(np.arange(f.n_cells), np.diff(np.asarray(f.cell_dt_off)))
    cols = [_up(f.dt_cat, np.int32), _up(f.dt_box, np.float64), _up(f.dt_flags, np.uint8),
            _up(np.asarray(f.cell_gt_off)[d_cell], np.int32), _up(mg, np.int32)]
    gcols = [_up(f.gt_cat, np.int32), _up(f.gt_box, np.float64),
             _up(gt_rng, np.uint32).view(torch.int32)]
    dt_counts = torch.full((n_rng, K, 7), -3, dtype=torch.int64, device=DEV)
    gt_counts = torch.full((n_rng, K, 3), -3, dtype=torch.int64, device=DEV)
    dt_type = torch.full((max(n_dt, 1), n_rng), 99, dtype=torch.uint8, device=DEV)
    same = torch.full((max(n_dt, 1), n_rng), -9, dtype=torch.int32, device=DEV)
    other = torch.full((max(n_dt, 1), n_rng), -9, dtype=torch.int32, device=DEV)
    held = torch.full((n_rng, max(n_gt, 1)), 7, dtype=torch.uint8, device=DEV)
    need = lib.taoamd_error_types_workspace(n_dt, n_gt, min(n_rng, 8))
    ws = wsguard.Guarded(need if ws_bytes is None else ws_bytes, DEV)
    head = [n_dt, n_gt, n_img, K, n_rng, slot, tb, *[c.data_ptr() for c in cols[:4]],
            cols[4].data_ptr(), n_rng * N_THR, *[c.data_ptr() for c in gcols],
            g_off.data_ptr(), g_rows.data_ptr(), d_off.data_ptr(), d_rows.data_ptr(),
            dt_counts.data_ptr(), gt_counts.data_ptr(), dt_type.data_ptr()]
    tail = [ws.data_ptr(), ws.nbytes, torch.cuda.current_stream().cuda_stream]
    if links:
        extra = [None if drop == i else x.data_ptr() for i, x in enumerate((same, other, held))]
        st = lib.taoamd_error_types_links(*head, *extra, *tail)
    else:
        st = lib.taoamd_error_types(*head, *tail)
    if status:
        torch.cuda.synchronize()
        return st
    _lib.check(st, "taoamd_error_types_links")
    ws.check()
    return dict(dt_counts=dt_counts.cpu().numpy(), gt_counts=gt_counts.cpu().numpy(),
                dt_type=dt_type[:n_dt].cpu().numpy(), link_same=same[:n_dt].cpu().numpy(),
                link_other=other[:n_dt].cpu().numpy(), held=held[:, :n_gt].cpu().numpy())


def _device_impact(n_cat, n_rng, dt_cat, score, dt_type, link_same, link_other, gt_cat, gt_rng,
                   held, status=False, ws_bytes=None, order=None):
    """taoamd_error_impact on bare tables, cat_off / order[] as the sort leaves
    them; the workspace is exactly the size reported, behind a guard band."""
    import torch
    lib = _lib.load()
    n_dt, n_gt = len(dt_cat), len(gt_cat)
    cat_off, srt = ref.sweep_order(dt_cat, score, n_cat)
    if order is not None:
        srt = order
    cols = [_up(cat_off, np.int32), _up(srt, np.int32), _up(score, np.float64),
            _up(dt_cat, np.int32), _up(np.asarray(dt_type).reshape(n_dt, n_rng), np.uint8),
            _up(np.asarray(link_same).reshape(n_dt, n_rng), np.int32),
            _up(np.asarray(link_other).reshape(n_dt, n_rng), np.int32),
            _up(gt_cat, np.int32), _up(gt_rng, np.uint32).view(torch.int32),
            _up(np.asarray(held).reshape(n_rng, n_gt), np.uint8)]
    P = torch.full((9, N_REC, n_cat, n_rng), -7.0, dtype=torch.float64, device=DEV)
    NG = torch.full((9, n_cat, n_rng), -7, dtype=torch.int32, device=DEV)
    need = lib.taoamd_error_impact_workspace(n_dt, n_gt, n_cat, min(n_rng, 8))
    ws = wsguard.Guarded(need if ws_bytes is None else ws_bytes, DEV)
    st = lib.taoamd_error_impact(
        n_dt, n_gt, n_cat, n_rng,
        *[c.data_ptr() for c in cols], P.data_ptr(), NG.data_ptr(), ws.data_ptr(), ws.nbytes,
        torch.cuda.current_stream().cuda_stream)
    if status:
        torch.cuda.synchronize()
        return st
    _lib.check(st, "taoamd_error_impact")
    ws.check()
    return dict(precision=P.cpu().numpy(), num_gt=NG.cpu().numpy().astype(np.int64))


def _impact_of(f, types, gt_rng, n_rng, **kw):
    return _device_impact(len(f.cat_ids), n_rng, f.dt_cat, f.dt_score, types["dt_type"],
                          types["link_same"], types["link_other"], f.gt_cat, gt_rng,
                          types["held"], **kw)


def _same(got, want):
    assert np.array_equal(got["num_gt"], want["num_gt"])
    assert np.array_equal(got["precision"], want["precision"])


def _same_links(got, want):
    assert np.array_equal(got["link_same"], want["link_same"])
    assert np.array_equal(got["link_other"], want["link_other"])
    assert np.array_equal(got["held"].astype(bool), want["held"])
    assert np.array_equal(got["dt_type"], want["types"]["dt_type"])
    assert np.array_equal(got["dt_counts"], want["types"]["dt_counts"])
    assert np.array_equal(got["gt_counts"], want["types"]["gt_counts"])


def test_abi_on_the_hand_written_table():
    f, dt_at, gt_at = et.make_flat(hand.N_IMG, hand.N_CAT, hand.DETS, hand.GTS)
    gt_rng, _ = orclib.ranges(f)
    thrs, rec = orclib.thresholds()
    mg = _device_match(f, gt_rng, 6)
    want = ref.error_impact(f, mg, gt_rng, thrs, 0, et.HAND_TB)
    types = _device_types(f, mg, gt_rng, 6, 0, et.HAND_TB)
    assert types["dt_type"][dt_at, 0].tolist() == et.HAND_TYPES_RNG0 + hand.NEW_TYPES_RNG0
    assert types["link_other"][dt_at[[29, 31, 30, 32, 4, 10]], 0].tolist() == \
        gt_at[[13, 13, 14, 14, 3, 4]].tolist()
    _same_links(types, want)
    got = _impact_of(f, types, gt_rng, 6)
    P = got["precision"][..., 0]
    # the literals of the host test, from the device
    assert np.array_equal(P[ref.F_LOC, :, 0], hand.expected(
        6, {0: (4, 4), 1: (4, 4), 2: (4, 4), 3: (4, 4), 4: (4, 4), 5: (6, 8), 6: (6, 8)}, rec))
    assert np.array_equal(P[ref.F_CLS, :, 4], hand.expected(2, {0: (1, 3), 1: (1, 3), 2: (2, 8)}, rec))
    assert np.array_equal(P[ref.F_CLS, :, 1], hand.expected(1, {0: (1, 2), 1: (1, 2)}, rec))
    assert (P[ref.F_MISS, :, 7] == -1).all() and (P[ref.BASE, :, 7] == 0).all()
    assert got["num_gt"][ref.F_MISS, :, 0].tolist() == [6, 1, 0, 4, 2, 1, 1, 0, 1]
    _same(got, want)


# ---------------------------------------------------------------------------
# random box tables: the shapes of the breakdown's own test -- every pairing of
# {0, 1, 63, 64, 65} ground truths and detections per image, 257 and 1025
# detections, ground truths around the pair kernel's LDS tile
# ---------------------------------------------------------------------------
SMALL = [0, 1, 63, 64, 65]
IMAGES = [(g, d) for g in SMALL for d in SMALL] + \
    [(5, 257), (40, 1025), (TILE - 1, 30), (TILE, 64), (TILE + 1, 65), (2 * TILE + 1, 130)]
N_CAT = 5
SETTINGS = ((0, 0.0), (5, 0.25), (0, 0.25))


def box_tables(n_rng, seed=None):
    """(flat, gt_rng): integer boxes on a coarse grid, so IoUs repeat and land on
    the thresholds.  A detection is, by chance, a ground truth's box (true
    positives and duplicates), a slice of it (LOC), either under another
    category (CLS, BOTH), or anything; scores come from few values, some NaN."""
    rng = np.random.default_rng(140 + n_rng if seed is None else seed)

    def box():
        x, y = rng.integers(0, 12, 2) * 2
        w, h = rng.choice([1, 2, 4, 8], 2)
        return [int(x), int(y), int(w), int(h)]
    dets, gts = [], []
    for u, (ng, nd) in enumerate(IMAGES):
        for _ in range(ng):
            gts.append((u, int(rng.integers(N_CAT)), box(), 1.0,
                        int(rng.choice([0, 0, 0, 0, 4]))))
        mine = gts[len(gts) - ng:]
        for _ in range(nd):
            cat, bx = int(rng.integers(N_CAT)), box()
            p = rng.random()
            if ng and p < 0.5:
                _, cat, bx, _, _ = mine[int(rng.integers(ng))]
                bx = list(bx)
                if p < 0.2 and bx[3] > 1:              # the upper half: IoU 0.5 or below
                    bx[3] //= 2
                if rng.random() < 0.3:
                    cat = int(rng.integers(N_CAT))
            score = float(rng.integers(0, 50)) / 50 if rng.random() > 0.02 else NAN
            dets.append((u, cat, bx, score, int(rng.choice([0, 0, 0, 1, 2]))))
    f, _, _ = et.make_flat(len(IMAGES), N_CAT, dets, gts)
    gt_rng = np.zeros(len(gts), np.uint32)
    for a in range(n_rng):
        gt_rng |= (rng.random(len(gts)) < 0.3).astype(np.uint32) << np.uint32(a)
    return f, gt_rng


@pytest.fixture(scope="module")
def random_boxes():
    """{n_rng: (flat, gt_rng, match_gt of taoamd_match, {(slot, tb): restatement})}"""
    out = {}
    thrs, _ = orclib.thresholds()
    for n_rng in (1, 6):
        f, gt_rng = box_tables(n_rng)
        mg = _device_match(f, gt_rng, n_rng)
        want = {(t, tb): ref.error_impact(f, mg, gt_rng, thrs, t, tb, n_rng)
                for t, tb in SETTINGS}
        for w in want.values():
            for v in w.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        out[n_rng] = (f, gt_rng, mg, want)
    return out


@pytest.mark.parametrize("slot,tb", SETTINGS)
@pytest.mark.parametrize("n_rng", [1, 6])
def test_links_and_sweep_on_seeded_random_boxes(random_boxes, n_rng, slot, tb):
    f, gt_rng, mg, want = random_boxes[n_rng]
    w = want[slot, tb]
    # the cases are there.  (tb = 0: an unmatched row is DUP or LOC, whatever it
    # overlaps -- no CLS row, so no adopted one, and three fixes change nothing)
    none = ("adopted",) if tb == 0 else ()
    idle = (ref.F_CLS, ref.F_BOTH, ref.F_BKG) if tb == 0 else ()
    for name in EVENTS:
        assert (w["events"][name] > 0) == (name not in none), name
    assert set(np.unique(w["types"]["dt_type"])) == set(range(4 if tb == 0 else 7))
    assert (w["link_same"] == -1).any() and (w["link_other"] == -1).any()
    P = w["precision"]
    for v in range(1, 9):
        assert (P[v] != P[0]).any() == (v not in idle), ref.FIXES[v]
    types = _device_types(f, mg, gt_rng, n_rng, slot, tb)
    _same_links(types, w)
    _same(_impact_of(f, types, gt_rng, n_rng), w)


def test_error_types_outputs_unchanged_after_a_links_call(random_boxes):
    f, gt_rng, mg, want = random_boxes[6]
    before = _device_types(f, mg, gt_rng, 6, 0, 0.0, links=False)
    _device_types(f, mg, gt_rng, 6, 5, 0.25)
    after = _device_types(f, mg, gt_rng, 6, 0, 0.0, links=False)
    for k in ("dt_counts", "gt_counts", "dt_type"):
        assert np.array_equal(before[k], after[k])
        assert np.array_equal(before[k], want[0, 0.0]["types"][k])
    # taoamd_error_types touched none of the tables of the links
    assert (after["link_same"] == -9).all() and (after["held"] == 7).all()


# ---------------------------------------------------------------------------
# bare random tables: the sweep is level-agnostic, so are its inputs.  Category
# lengths around the wavefront and around the rows of a sweep step.
# ---------------------------------------------------------------------------
LENGTHS = [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]


def bare_tables(n_rng, seed=None):
    rng = np.random.default_rng(240 + n_rng if seed is None else seed)
    K = len(LENGTHS)
    dt_cat = rng.permutation(np.repeat(np.arange(K), LENGTHS))
    n_dt, n_gt = len(dt_cat), 12 * K
    gt_cat = rng.integers(0, K, n_gt)
    gt_rng = np.zeros(n_gt, np.uint32)
    for a in range(n_rng):
        gt_rng |= (rng.random(n_gt) < 0.25).astype(np.uint32) << np.uint32(a)
    held = rng.random((n_rng, n_gt)) < 0.4
    score = rng.choice([0.0, -0.0, 0.25, 0.5, 0.5, 0.75, 1.0, -1.0, NAN, np.inf, -np.inf, 1e300],
                       n_dt)
    dt_type = rng.choice([0, 0, 1, 2, 3, 3, 3, 4, 4, 5, 6, 9], (n_dt, n_rng)).astype(np.uint8)
    # links: mostly a ground truth of the row's category / of another, some
    # none, some outside the table
    by_cat = [np.flatnonzero(gt_cat == c) for c in range(K)]
    link_same = -np.ones((n_dt, n_rng), np.int64)
    link_other = -np.ones((n_dt, n_rng), np.int64)
    for d in range(n_dt):
        for a in range(n_rng):
            own = by_cat[dt_cat[d]]
            if len(own) and rng.random() < 0.8:
                link_same[d, a] = own[rng.integers(len(own))]
            if rng.random() < 0.8:
                link_other[d, a] = rng.integers(n_gt)
    wild = rng.random((n_dt, n_rng)) < 0.02
    link_same[wild] = rng.choice([n_gt, n_gt + 5, -7, 2 ** 31 - 1], int(wild.sum()))
    link_other[wild] = rng.choice([n_gt, -2, -2 ** 31], int(wild.sum()))
    return dict(n_cat=K, n_rng=n_rng, dt_cat=dt_cat, score=score, dt_type=dt_type,
                link_same=link_same, link_other=link_other, gt_cat=gt_cat, gt_rng=gt_rng,
                held=held)


@pytest.fixture(scope="module")
def random_bare():
    out = {}
    rec = orclib.thresholds()[1]
    for n_rng in (1, 6):
        t = bare_tables(n_rng)
        out[n_rng] = (t, ref.impact_tables(rec_thrs=rec, **t))
    return out


@pytest.mark.parametrize("n_rng", [1, 6])
def test_sweep_on_seeded_bare_tables(random_bare, n_rng):
    t, want = random_bare[n_rng]
    for name in EVENTS:
        assert want["events"][name] > 0, name
    assert np.bincount(t["dt_cat"], minlength=t["n_cat"]).tolist() == LENGTHS
    for v in range(1, 9):
        assert (want["precision"][v] != want["precision"][0]).any(), ref.FIXES[v]
    # an empty category adopts rows; so does the longest
    assert (want["precision"][ref.F_CLS, :, 0] > 0).any()
    _same(_device_impact(**t), want)


def test_sweep_on_a_long_category():
    """300 001 rows of one category: more than a thousand steps of one
    workgroup, the counts carried from step to step; a short one beside it,
    whose CLS rows the long one adopts."""
    rng = np.random.default_rng(77)
    n_long, n_gt = 300001, 60
    dt_cat = np.r_[np.zeros(n_long, np.int64), np.ones(300, np.int64)]
    n_dt = len(dt_cat)
    gt_cat = np.r_[np.zeros(n_gt - 4, np.int64), np.ones(4, np.int64)]
    score = rng.integers(0, 5000, n_dt) / 5000.0
    dt_type = rng.choice([0, 1, 2, 3, 4, 5, 6, 6, 6, 6], (n_dt, 1)).astype(np.uint8)
    dt_type[rng.random(n_dt) < 0.9995, 0] = et.BKG            # few true positives
    dt_type[rng.integers(0, n_dt, 40), 0] = et.TP
    dt_type[rng.integers(0, n_dt, 200), 0] = et.LOC
    dt_type[rng.integers(0, n_dt, 200), 0] = et.CLS
    dt_type[n_long:, 0] = rng.choice([0, 3, 4, 4, 6], 300)   # the long one adopts their CLS rows
    # (links name the first 40 ground truths only: the others stay unlinked)
    link_same = np.where(dt_cat == 0, rng.integers(0, 40, n_dt),
                         rng.integers(n_gt - 4, n_gt, n_dt)).reshape(-1, 1)
    link_other = np.where(dt_cat == 0, rng.integers(n_gt - 4, n_gt, n_dt),
                          rng.integers(0, 40, n_dt)).reshape(-1, 1)
    t = dict(n_cat=2, n_rng=1, dt_cat=dt_cat, score=score, dt_type=dt_type, link_same=link_same,
             link_other=link_other, gt_cat=gt_cat, gt_rng=np.zeros(n_gt, np.uint32),
             held=rng.random((1, n_gt)) < 0.5)
    want = ref.impact_tables(rec_thrs=orclib.thresholds()[1], **t)
    for name in EVENTS:
        assert want["events"][name] > 0, name
    for v in range(1, 9):
        assert (want["precision"][v, :, 0] != want["precision"][0, :, 0]).any(), ref.FIXES[v]
    _same(_device_impact(**t), want)


def test_sweep_with_the_workspace_base_moved_by_8_bytes(random_bare, monkeypatch):
    monkeypatch.setattr(wsguard, "SHIFT", 8)
    t, want = random_bare[6]
    _same(_device_impact(**t), want)


def test_links_with_the_workspace_base_moved_by_8_bytes(random_boxes, monkeypatch):
    monkeypatch.setattr(wsguard, "SHIFT", 8)
    f, gt_rng, mg, want = random_boxes[6]
    _same_links(_device_types(f, mg, gt_rng, 6, 5, 0.25), want[5, 0.25])


def test_sweep_skips_rows_outside_the_table(random_bare):
    """order[] entries outside [0, n_dt) are rows of no list, never dereferenced."""
    t, _ = random_bare[1]
    cat_off, order = ref.sweep_order(t["dt_cat"], t["score"], t["n_cat"])
    gone = np.arange(len(order)) % 7 == 3
    broken = order.copy()
    broken[gone] = np.where(np.arange(gone.sum()) % 2 == 0, -1, len(order))
    ty = t["dt_type"].copy()
    ty[order[gone]] = 9                      # the same rows, dropped by their type byte
    # (no adopted row: its place is found by bisection over order[], which such
    # entries leave without an order)
    ty[ty == et.CLS] = et.BOTH
    rec = orclib.thresholds()[1]
    want = ref.impact_tables(rec_thrs=rec, **{**t, "dt_type": ty})
    _same(_device_impact(order=broken, **{**t, "dt_type": ty}), want)


def test_abi_error_paths(random_bare, random_boxes):
    t, _ = random_bare[1]
    lib = _lib.load()
    assert _device_impact(status=True, **t) == 0
    assert _device_impact(status=True, ws_bytes=lib.taoamd_error_impact_workspace(
        len(t["dt_cat"]), len(t["gt_cat"]), t["n_cat"], 1) - 1, **t) == 4
    import torch
    p = torch.zeros(64, dtype=torch.int64, device=DEV).data_ptr()
    need = lib.taoamd_error_impact_workspace(0, 0, 3, 1)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call(n_dt=0, n_gt=0, n_cat=3, n_rng=1, cat_off=p, prec=p):
        st = lib.taoamd_error_impact(n_dt, n_gt, n_cat, n_rng, cat_off, None, None, None, None,
                                     None, None, None, None, None, prec, p, ws.data_ptr(), need,
                                     None)
        torch.cuda.synchronize()
        return st
    assert call(n_rng=0) == 2 and call(n_rng=9) == 2 and call(n_cat=0) == 2
    assert call(n_dt=-1) == 2 and call(n_gt=2 ** 31) == 2
    assert call(cat_off=None) == 2 and call(prec=None) == 2
    assert call(n_dt=1) == 2 and call(n_gt=1) == 2           # tables missing
    f, gt_rng, mg, _ = random_boxes[1]
    links = lambda **kw: _device_types(f, mg, gt_rng, kw.pop("n_rng", 1),  # noqa: E731
                                       kw.pop("slot", 0), kw.pop("tb", 0.1), status=True, **kw)
    assert links(slot=10) == 2 and links(tb=0.5) == 2 and links(n_rng=9) == 2
    assert links(drop=0) == 2 and links(drop=1) == 2 and links(drop=2) == 2
    need = lib.taoamd_error_types_workspace(int(f.cell_dt_off[-1]), int(f.cell_gt_off[-1]), 1)
    assert links(ws_bytes=need - 1) == 4
    assert links() == 0


def test_sweep_without_rows_or_ground_truths():
    rec = orclib.thresholds()[1]
    none = np.zeros((0, 1), np.int64)
    t = dict(n_cat=3, n_rng=1, dt_cat=np.zeros(0, np.int64), score=np.zeros(0),
             dt_type=np.zeros((0, 1), np.uint8), link_same=none, link_other=none,
             gt_cat=np.array([0, 0, 2]), gt_rng=np.array([0, 1, 0], np.uint32),
             held=np.zeros((1, 3), bool))
    want = ref.impact_tables(rec_thrs=rec, **t)
    got = _device_impact(**t)
    _same(got, want)
    assert got["num_gt"][0, :, 0].tolist() == [1, 0, 1]
    assert (got["precision"][0, :, 0] == 0).all() and (got["precision"][0, :, 1] == -1).all()
    t.update(gt_cat=np.zeros(0, np.int64), gt_rng=np.zeros(0, np.uint32),
             held=np.zeros((1, 0), bool), dt_cat=np.array([1, 1]), score=np.array([0.5, 0.25]),
             dt_type=np.array([[0], [6]], np.uint8), link_same=-np.ones((2, 1), np.int64),
             link_other=-np.ones((2, 1), np.int64))
    got = _device_impact(**t)
    _same(got, ref.impact_tables(rec_thrs=rec, **t))
    assert (got["precision"] == -1).all()


# ---------------------------------------------------------------------------
# the class API
# ---------------------------------------------------------------------------
def _lvis(name, tmp_path, iou_type="bbox", pred=None):
    from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
    if pred is not None:
        return LVISEval(path(name, "gt.json"), path(name, pred), iou_type)
    gt, dt = input_paths(name, tmp_path)
    return LVISEval(gt, dt, iou_type)


def _restated(ev, iou_thr, bg_thr):
    """The restatement on the evaluator's own tables: match indices and range
    masks of a detail-mode pass under the evaluator's constants, the kernels'
    range slots put in the caller's order, the recall thresholds the caller's."""
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
    thrs = orclib.thresholds()[0] if c is None else c.thr_blocks[0][1]
    i = int(np.where(iou_thr == np.asarray(ev.params.iou_thrs))[0][0])
    slot = i if c is None else int(np.where(c.thr_blocks[0][0] == i)[0][0])
    assert thrs[slot] == iou_thr
    want = ref.error_impact(run.flat, mg, gt_rng, thrs, slot, bg_thr,
                            rec_thrs=np.asarray(ev.params.rec_thrs, dtype=np.float64))
    P = want["precision"]
    if len(ev.params.visibility_rng) != 6:
        ks = list(range(len(ev.params.visibility_rng) - 1)) + [5]
        P = P[..., ks]
    cats = np.asarray(run.flat.cat_ids).tolist()
    pos = [cats.index(int(c)) for c in ev.params.cat_ids]
    return np.ascontiguousarray(P[:, :, pos]), want["events"]


def _check_class_api(ev, iou_thr, bg_thr):
    from tao_amodal_amd.evaluation._core import masked_mean
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.error_impact(iou_thr, bg_thr)
    ev.evaluate()
    want, events = _restated(ev, iou_thr, bg_thr)
    got = ev.error_impact(iou_thr, bg_thr)
    assert got["fixes"] == list(ref.FIXES) and got["rng_lbl"] == ev.params.visibility_rng_lbl
    n_rng, K, R = len(ev.params.visibility_rng), len(ev.params.cat_ids), len(ev.params.rec_thrs)
    assert got["precision"].shape == (9, R, K, n_rng) and got["precision"].dtype == np.float64
    assert np.array_equal(got["precision"], want)
    assert got["ap"].shape == (9, n_rng) and got["dap"].shape == (8, n_rng)
    for v in range(9):
        for a in range(n_rng):
            assert got["ap"][v, a] == masked_mean(want[v, :, :, a])
    assert np.array_equal(got["dap"], got["ap"][1:] - got["ap"][0])
    assert ev.error_impact(iou_thr, bg_thr)["precision"] is got["precision"]       # cached
    # the breakdown next to it is the one the impact was computed from
    ev.error_types(iou_thr, bg_thr)
    ev.accumulate()
    lines = ev.impact_lines(iou_thr, bg_thr)
    assert len(lines) == 2 + n_rng and all(isinstance(x, str) for x in lines)
    assert lines[1].split() == ["AP"] + ["d" + x for x in ref.FIXES[1:]]
    assert lines[2].split()[-9:] == ["%.4f" % v for v in
                                     np.concatenate([got["ap"][:1, 0], got["dap"][:, 0]])]
    return got, events


def _has_hidden_id(name, tmp_path):
    with open(input_paths(name, tmp_path)[0]) as fh:
        return any(a["id"] == 0 for a in json.load(fh)["annotations"])


FIXTURES = ["f1", "f2", "f3", "f4", "f5", "f6", "f7", "f8", "f9", "f10"]


@pytest.mark.parametrize("name", FIXTURES)
def test_class_api_on_the_fixtures(name, tmp_path):
    ev = _lvis(name, tmp_path)
    got, _ = _check_class_api(ev, 0.5, 0.1)
    t = int(np.where(0.5 == np.asarray(ev.params.iou_thrs))[0][0])
    if _has_hidden_id(name, tmp_path):
        return
    # BASE is accumulate()'s table, its mean the AP summarize() reports
    assert np.array_equal(got["precision"][0], ev.eval["precision"][t])
    for a, lbl in enumerate(ev.params.visibility_rng_lbl):
        assert got["ap"][0, a] == ev._summarize("ap", 0.5, lbl)


def test_some_fixture_has_no_hidden_ground_truth_id(tmp_path):
    plain = [name for name in FIXTURES if not _has_hidden_id(name, tmp_path)]
    assert plain and len(plain) < len(FIXTURES)


def test_class_api_at_another_threshold():
    ev = _lvis("f1", None, pred="pred.json")
    got, events = _check_class_api(ev, ev.params.iou_thrs[5], 0.3)
    assert np.array_equal(got["precision"][0], ev.eval["precision"][5])
    assert events["winner"] > 0


@pytest.mark.parametrize("case,iou_thr", [("few", 0.75), ("few", 0.3), ("ranges3", 0.5),
                                          ("unsorted_rec", 0.5)])
def test_class_api_under_edited_constants_of_one_block(case, iou_thr):
    """Thresholds in the caller's unsorted order; a visibility_rng of 3 ranges
    (kernel slots 0, 1 and the out-of-frame one); recall thresholds unsorted."""
    ev = _lvis("f1", None, pred="pred.json")
    edit(ev.params, cases()[case], "lvis")
    got, _ = _check_class_api(ev, iou_thr, 0.1)
    t = int(np.where(iou_thr == np.asarray(ev.params.iou_thrs))[0][0])
    assert np.array_equal(got["precision"][0], ev.eval["precision"][t])
    assert got["precision"].shape[3] == len(ev.params.visibility_rng)


def test_class_api_on_a_params_subset():
    ev = _lvis("f1", None, pred="pred.json")
    ev.params.img_ids = ev.params.img_ids[::2]
    ev.params.cat_ids = [ev.params.cat_ids[i] for i in (4, 0, 2)]
    got, _ = _check_class_api(ev, 0.5, 0.1)
    assert got["precision"].shape[2] == 3
    assert np.array_equal(got["precision"][0], ev.eval["precision"][0])


def test_class_api_refusals():
    ev = _lvis("f1", None, pred="pred.json")
    ev.evaluate()
    with pytest.raises(ValueError, match="not one of params.iou_thrs"):
        ev.error_impact(0.55000001)
    for bad in (0.5, 0.7, -0.1):
        with pytest.raises(ValueError, match="bg_thr"):
            ev.error_impact(0.5, bad)
    from tao_amodal_amd import engine
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_error_impact(ev._run.dp, ev._run.ws, 10, 0.1)
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_error_impact(ev._run.dp, ev._run.ws, 0, 0.5)
    many = _lvis("f1", None, pred="pred.json")
    edit(many.params, cases()["many"], "lvis")
    many.evaluate()
    with pytest.raises(NotImplementedError, match=r"error_types\(\) is kept for up to 10 IoU"):
        many.error_impact(many.params.iou_thrs[9])
    wide = _lvis("f1", None, pred="pred.json")
    edit(wide.params, cases()["ranges8"], "lvis")
    wide.evaluate()
    with pytest.raises(NotImplementedError, match="one block of ranges"):
        wide.error_impact(0.5)
    pooled = _lvis("f1", None, pred="pred.json")
    pooled.params.use_cats = 0
    pooled.evaluate()
    with pytest.raises(NotImplementedError, match="use_cats = 0"):
        pooled.error_impact(0.5)
    segm = _lvis("f6", None, "segm", pred="pred_rle.json")
    segm.evaluate()
    with pytest.raises(NotImplementedError, match="iou_type='segm'"):
        segm.error_impact(0.5)
    from tao_amodal_amd.evaluation._dist import DistRun
    with pytest.raises(NotImplementedError, match=r"error_types\(\) in a multi-GPU run"):
        DistRun.__new__(DistRun).impact_table(0, 0.1)
