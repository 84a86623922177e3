"""-m gpu: the image-level error breakdown (taoamd_error_types,
engine.stage_error_types, LVISEval.error_types) against the numpy restatement of
tests/error_types_ref.py.  The restatement's IoUs are the C oracle's bbIou, the
kernel's arithmetic: every comparison is exact."""
import sys

import numpy as np
import pytest

import error_types_ref as ref
import orclib
import wsguard
from goldenio import GOLDEN as GOLDEN_DIR, input_paths, path
from tao_amodal_amd import _lib

sys.path.insert(0, GOLDEN_DIR)
from constants_cases import cases, edit  # noqa: E402

pytestmark = pytest.mark.gpu

N_THR = _lib.N_THR
TILE = _lib.ERROR_TYPES_TILE
DEV = "cuda:0"


def _up(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], dtype=dtype)
    return torch.from_numpy(a).to(DEV)


def _device_match(f, gt_rng, n_rng):
    """match_gt[n_dt, n_rng * 10] of taoamd_match itself (one wavefront per cell)."""
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


def _device_error_types(f, mg, gt_rng, n_rng, slot, tb, per_detection=True, status=False,
                        ws_bytes=None):
    """taoamd_error_types on a Flat; the workspace is exactly the size reported,
    behind a guard band."""
    import torch
    lib = _lib.load()
    n_dt, n_gt = int(f.cell_dt_off[-1]), int(f.cell_gt_off[-1])
    n_img, K = len(f.img_ids), len(f.cat_ids)
    d_img, g_img = ref.units(f)

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
    need = lib.taoamd_error_types_workspace(n_dt, n_gt, min(n_rng, 8))
    ws = wsguard.Guarded(need if ws_bytes is None else ws_bytes, DEV)
    st = lib.taoamd_error_types(
        n_dt, n_gt, n_img, K, n_rng, slot, tb, *[c.data_ptr() for c in cols[:4]],
        cols[4].data_ptr(), n_rng * N_THR, *[c.data_ptr() for c in gcols],
        g_off.data_ptr(), g_rows.data_ptr(), d_off.data_ptr(), d_rows.data_ptr(),
        dt_counts.data_ptr(), gt_counts.data_ptr(),
        dt_type.data_ptr() if per_detection else None, ws.data_ptr(), ws.nbytes,
        torch.cuda.current_stream().cuda_stream)
    if status:
        torch.cuda.synchronize()
        return st
    _lib.check(st, "taoamd_error_types")
    ws.check()
    return dict(dt_counts=dt_counts.cpu().numpy(), gt_counts=gt_counts.cpu().numpy(),
                dt_type=dt_type[:n_dt].cpu().numpy() if per_detection else None)


def _same(got, want):
    assert np.array_equal(got["dt_counts"], want["dt_counts"])
    assert np.array_equal(got["gt_counts"], want["gt_counts"])
    if got["dt_type"] is not None:
        assert np.array_equal(got["dt_type"], want["dt_type"])


def test_abi_on_the_hand_written_table():
    f, dt_at, gt_at = ref.hand_flat()
    gt_rng, _ = orclib.ranges(f)
    thrs, _ = orclib.thresholds()
    mg = _device_match(f, gt_rng, 6)
    got = _device_error_types(f, mg, gt_rng, 6, 0, ref.HAND_TB)
    assert got["dt_type"][dt_at, 0].tolist() == ref.HAND_TYPES_RNG0
    assert got["dt_type"][dt_at, 1].tolist() == ref.HAND_TYPES_RNG1
    assert got["dt_counts"][0].tolist() == ref.HAND_DT_COUNTS_RNG0
    assert got["gt_counts"][0].tolist() == ref.HAND_GT_COUNTS_RNG0
    _same(got, ref.error_types(f, mg, gt_rng, thrs, 0, ref.HAND_TB))
    # just above tb the rows pinned at exactly tb fall to BKG
    up = _device_error_types(f, mg, gt_rng, 6, 0, 0.125 + 2.0 ** -50)
    assert up["dt_type"][dt_at[[9, 11]], 0].tolist() == [ref.BKG, ref.BKG]
    _same(up, ref.error_types(f, mg, gt_rng, thrs, 0, 0.125 + 2.0 ** -50))
    # another slot: tf = 0.75
    _same(_device_error_types(f, mg, gt_rng, 6, 5, 0.3),
          ref.error_types(f, mg, gt_rng, thrs, 5, 0.3))


# (ground truths, detections) per image: every pairing of {0, 1, 63, 64, 65}, then
# 257 and 1025 detections (a workgroup's lanes loop), then ground truths one
# below, at and above the kernel's LDS tile and at twice the tile plus one
SMALL = [0, 1, 63, 64, 65]
IMAGES = [(g, d) for g in SMALL for d in SMALL] + \
    [(5, 257), (40, 1025), (TILE - 1, 30), (TILE, 64), (TILE + 1, 65), (2 * TILE + 1, 130)]
N_CAT = 5


@pytest.fixture(scope="module")
def random_tables():
    """{n_rng: (flat, gt_rng, match_gt of taoamd_match, restatement at (slot 0,
    tb 0.1) and (slot 5, tb 0.25))}: integer boxes on a coarse grid, so IoUs repeat
    and land on the thresholds; ground truths spread over the categories."""
    out = {}
    for n_rng in (1, 6):
        rng = np.random.default_rng(40 + n_rng)

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
                if ng and rng.random() < 0.3:          # on a ground truth: TPs and DUPs
                    _, cat, bx, _, _ = mine[int(rng.integers(ng))]
                dets.append((u, cat, bx, float(rng.integers(0, 50)) / 50,
                             int(rng.choice([0, 0, 0, 1, 2]))))
        f, _, _ = ref.make_flat(len(IMAGES), N_CAT, dets, gts)
        n_gt = len(gts)
        gt_rng = np.zeros(n_gt, np.uint32)
        for a in range(n_rng):
            gt_rng |= (rng.random(n_gt) < 0.3).astype(np.uint32) << np.uint32(a)
        mg = _device_match(f, gt_rng, n_rng)
        thrs, _ = orclib.thresholds()
        want = {(t, tb): ref.error_types(f, mg, gt_rng, thrs, t, tb, n_rng)
                for t, tb in ((0, 0.1), (5, 0.25))}
        for w in want.values():
            for v in w.values():
                v.setflags(write=False)
        out[n_rng] = (f, gt_rng, mg, want)
    return out


@pytest.mark.parametrize("slot,tb", [(0, 0.1), (5, 0.25)])
@pytest.mark.parametrize("n_rng", [1, 6])
def test_abi_on_seeded_random_tables(random_tables, n_rng, slot, tb):
    f, gt_rng, mg, want = random_tables[n_rng]
    w = want[slot, tb]
    # the cases are there: every type, ties at both thresholds, matches in every image size
    assert set(np.unique(w["dt_type"])) == set(range(7))
    assert (mg >= 0).any() and (mg == -1).any() and (mg >= -1).all()
    if slot == 0:       # (no IoU of these boxes is 0.75: their areas are powers of two)
        assert (w["s"] == 0.5).any() and (w["o"] == 0.5).any()
    else:
        assert (w["s"] == tb).any() and (w["o"] == tb).any()
    assert w["gt_counts"][..., 2].any()
    _same(_device_error_types(f, mg, gt_rng, n_rng, slot, tb), w)
    # the stated consequence: an unmatched row with s >= tf points at a held ground truth
    assert (w["dt_type"] == ref.DUP).sum() > 20
    for a in range(n_rng):
        dup = np.flatnonzero(w["dt_type"][:, a] == ref.DUP)
        assert w["hit"][a, w["arg"][dup, a]].all()


def test_abi_counts_do_not_depend_on_dt_type(random_tables):
    f, gt_rng, mg, want = random_tables[6]
    got = _device_error_types(f, mg, gt_rng, 6, 0, 0.1, per_detection=False)
    assert got["dt_type"] is None
    _same(got, want[0, 0.1])


def test_abi_with_the_workspace_base_moved_by_8_bytes(random_tables, monkeypatch):
    monkeypatch.setattr(wsguard, "SHIFT", 8)
    f, gt_rng, mg, want = random_tables[6]
    _same(_device_error_types(f, mg, gt_rng, 6, 5, 0.25), want[5, 0.25])


def test_abi_error_paths(random_tables):
    f, gt_rng, mg, _ = random_tables[1]
    lib = _lib.load()
    call = lambda **kw: _device_error_types(f, mg, gt_rng, kw.pop("n_rng", 1),  # noqa: E731
                                            kw.pop("slot", 0), kw.pop("tb", 0.1),
                                            status=True, **kw)
    assert call(slot=10) == 2 and call(slot=-1) == 2
    assert call(tb=0.5) == 2 and call(tb=0.9) == 2 and call(tb=-0.1) == 2
    assert call(n_rng=9) == 2
    need = lib.taoamd_error_types_workspace(int(f.cell_dt_off[-1]), int(f.cell_gt_off[-1]), 1)
    assert call(ws_bytes=need - 1) == 4
    assert call() == 0


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
    masks of a detail-mode pass under the evaluator's constants, the kernel's
    range slots put in the caller's order."""
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
    want = ref.error_types(run.flat, mg, gt_rng, thrs, slot, bg_thr)
    want = {k: want[k] for k in ("dt_counts", "gt_counts", "dt_type")}
    if len(ev.params.visibility_rng) != 6:
        # the kernels' slots of the caller's ranges: its visibility ranges from
        # slot 0 on, its last range in the out-of-frame slot 5
        ks = list(range(len(ev.params.visibility_rng) - 1)) + [5]
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
    assert got["rng_lbl"] == ev.params.visibility_rng_lbl
    n_rng, K = len(ev.params.visibility_rng), len(ev.params.cat_ids)
    assert got["dt_counts"].shape == (n_rng, K, 7) and got["dt_counts"].dtype == np.int64
    assert got["gt_counts"].shape == (n_rng, K, 3)
    assert np.array_equal(got["dt_counts"], want["dt_counts"])
    assert np.array_equal(got["gt_counts"], want["gt_counts"])
    assert ev.error_types(iou_thr, bg_thr)["dt_counts"] is got["dt_counts"]     # cached
    per = ev.error_types(iou_thr, bg_thr, per_detection=True)
    rows, types = per["dt_type"]
    assert np.array_equal(rows, np.asarray(ev._run.flat.dt_row))
    assert np.array_equal(types, want["dt_type"])
    assert np.array_equal(per["dt_counts"], want["dt_counts"])
    # accumulate() after it: the rows of the pass are as the match left them
    ev.accumulate()
    lines = ev.error_lines(iou_thr, bg_thr)
    assert len(lines) == 2 + n_rng and all(isinstance(x, str) for x in lines)
    assert lines[2].split()[-10:] == [str(int(v)) for v in np.concatenate(
        [want["dt_counts"][0].sum(0), want["gt_counts"][0].sum(0)])]
    return got


@pytest.mark.parametrize("name", ["f1", "f2", "f3", "f4", "f5", "f6", "f7", "f8", "f9", "f10"])
def test_class_api_on_the_fixtures(name, tmp_path):
    ev = _lvis(name, tmp_path)
    got = _check_class_api(ev, 0.5, 0.1)
    if name in ("f1", "f2", "f4", "f9"):
        from goldenio import load_eval
        p = load_eval(name)["lvis"][0]
        assert np.array_equal(ev.eval["precision"], p)
        assert got["dt_counts"].sum() == 6 * ev._run.dp.n_dt


def test_class_api_at_another_threshold():
    ev = _lvis("f1", None, pred="pred.json")
    _check_class_api(ev, ev.params.iou_thrs[5], 0.3)


@pytest.mark.parametrize("case,iou_thr", [("few", 0.75), ("few", 0.3), ("ranges3", 0.5)])
def test_class_api_under_edited_constants_of_one_block(case, iou_thr):
    """Thresholds in the caller's unsorted order; a visibility_rng of 3 ranges
    (kernel slots 0, 1 and the out-of-frame one)."""
    ev = _lvis("f1", None, pred="pred.json")
    edit(ev.params, cases()[case], "lvis")
    got = _check_class_api(ev, iou_thr, 0.1)
    assert got["dt_counts"].shape[0] == len(ev.params.visibility_rng)
    if case == "ranges3":
        # a second threshold: the pass evaluate() left out is not run again
        ws = ev._run.ws
        before = ws.err_match_gt.data_ptr(), ws.err_match_gt.clone()
        want = _restated(ev, ev.params.iou_thrs[5], 0.2)
        again = ev.error_types(ev.params.iou_thrs[5], 0.2)
        assert np.array_equal(again["dt_counts"], want["dt_counts"])
        assert np.array_equal(again["gt_counts"], want["gt_counts"])
        assert ws.err_match_gt.data_ptr() == before[0] and bool((ws.err_match_gt == before[1]).all())


def test_class_api_after_accumulate_leaves_the_rows_as_they_were():
    """The usual order: evaluate(), accumulate(), then a first error_types() --
    which runs the match once more for its indices.  The rows eval["scores"] is
    computed from afterwards are those of before."""
    ref_ev = _lvis("f1", None, pred="pred.json")
    ref_ev.evaluate()
    ref_ev.accumulate()
    scores = ref_ev.score_at_recall().copy()
    ev = _lvis("f1", None, pred="pred.json")
    ev.evaluate()
    ev.accumulate()
    rows = ev._run.ws.rows.clone()
    want = _restated(ev, 0.5, 0.1)
    got = ev.error_types(0.5, 0.1, per_detection=True)
    assert np.array_equal(got["dt_counts"], want["dt_counts"])
    assert np.array_equal(got["gt_counts"], want["gt_counts"])
    assert np.array_equal(got["dt_type"][1], want["dt_type"])
    assert bool((ev._run.ws.rows == rows).all())
    assert np.array_equal(ev.score_at_recall(), scores)
    assert (scores > 0).any()


def test_class_api_on_a_params_subset():
    """params.img_ids / cat_ids edited: the tables are those of the remaining
    images, the category axis is in the caller's order."""
    ev = _lvis("f1", None, pred="pred.json")
    ev.params.img_ids = ev.params.img_ids[::2]
    ev.params.cat_ids = [ev.params.cat_ids[i] for i in (4, 0, 2)]
    whole = _lvis("f1", None, pred="pred.json")
    whole.evaluate()
    got = _check_class_api(ev, 0.5, 0.1)
    assert got["dt_counts"].shape[1] == 3 and got["dt_counts"].sum() > 0
    assert ev._run.dp.n_dt < whole._run.dp.n_dt


def test_class_api_refusals():
    ev = _lvis("f1", None, pred="pred.json")
    ev.evaluate()
    with pytest.raises(ValueError, match="not one of params.iou_thrs"):
        ev.error_types(0.55000001)
    for bad in (0.5, 0.7, -0.1):
        with pytest.raises(ValueError, match="bg_thr"):
            ev.error_types(0.5, bad)
    from tao_amodal_amd import engine
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_error_types(ev._run.dp, ev._run.ws, 10, 0.1)
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_error_types(ev._run.dp, ev._run.ws, 0, 0.5)
    many = _lvis("f1", None, pred="pred.json")
    edit(many.params, cases()["many"], "lvis")
    many.evaluate()
    with pytest.raises(NotImplementedError, match=r"error_types\(\) is kept for up to 10 IoU"):
        many.error_types(many.params.iou_thrs[9])
    wide = _lvis("f1", None, pred="pred.json")
    edit(wide.params, cases()["ranges8"], "lvis")
    wide.evaluate()
    with pytest.raises(NotImplementedError, match="one block of ranges"):
        wide.error_types(0.5)
    pooled = _lvis("f1", None, pred="pred.json")
    pooled.params.use_cats = 0
    pooled.evaluate()
    with pytest.raises(NotImplementedError, match="use_cats = 0"):
        pooled.error_types(0.5)
    segm = _lvis("f6", None, "segm", pred="pred_rle.json")
    segm.evaluate()
    with pytest.raises(NotImplementedError, match="iou_type='segm'"):
        segm.error_types(0.5)
