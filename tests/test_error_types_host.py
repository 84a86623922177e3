"""The image-level error breakdown without a GPU: the numpy restatement
(tests/error_types_ref.py) on a hand-written table with literal expectations,
on the recorded fixtures with the Python oracle's matches, and the C ABI's new
symbols and refusals."""
import os
import re

import numpy as np
import pytest

import error_types_ref as ref
import orclib
from goldenio import load_eval, load_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["f1", "f2", "f3", "f4", "f5", "f7", "f9", "f10"]
GT_ID_HIDDEN = 4


def _oracle_tables(f):
    gt_rng, dt_rng = orclib.ranges(f)
    _, _, mg, _ = orclib.match(f, gt_rng, dt_rng)
    return gt_rng, mg


def test_hand_written_table_one_detection_of_each_type():
    f, dt_at, gt_at = ref.hand_flat()
    gt_rng, mg = _oracle_tables(f)
    thrs, _ = orclib.thresholds()
    assert thrs[0] == 0.5
    # the two pinned IoUs are exact in the oracle's arithmetic
    assert orclib.bb_iou([[0, 0, 2, 1]], [[0, 0, 1, 1]])[0, 0] == 0.5
    assert orclib.bb_iou([[10, 0, 1, 1]], [[10, 0, 4, 2]])[0, 0] == 0.125
    got = ref.error_types(f, mg, gt_rng, thrs, 0, ref.HAND_TB)
    assert got["dt_type"][dt_at, 0].tolist() == ref.HAND_TYPES_RNG0
    assert got["dt_type"][dt_at, 1].tolist() == ref.HAND_TYPES_RNG1
    assert got["dt_type"][dt_at[:7], 0].tolist() == list(range(7))   # image 0: each type once
    assert got["dt_counts"][0].tolist() == ref.HAND_DT_COUNTS_RNG0
    assert got["gt_counts"][0].tolist() == ref.HAND_GT_COUNTS_RNG0
    # fully visible: range 3 = range 0; nothing is evaluated in 1, 2, 4, 5
    assert np.array_equal(got["dt_counts"][3], got["dt_counts"][0])
    assert np.array_equal(got["gt_counts"][3], got["gt_counts"][0])
    assert not got["gt_counts"][[1, 2, 4, 5]].any()
    # >= at both thresholds: just above either, the four pinned rows fall a class
    up = ref.error_types(f, mg, gt_rng, thrs, 0, 0.125 + 2.0 ** -50)
    assert up["dt_type"][dt_at[[9, 11]], 0].tolist() == [ref.BKG, ref.BKG]
    assert up["gt_counts"][0, 0].tolist() == [6, 3, 2]
    thr_up = thrs.copy()
    thr_up[1] = 0.5 + 2.0 ** -50
    gt_rng1, mg1 = gt_rng, mg.copy()
    mg1[:, 1::10] = mg[:, 0::10]
    mg1[dt_at[7], 1::10] = -1               # (IoU 0.5 is below it: no match)
    at = ref.error_types(f, mg1, gt_rng1, thr_up, 1, ref.HAND_TB)
    assert at["dt_type"][dt_at[[7, 8, 10]], 0].tolist() == [ref.LOC, ref.LOC, ref.BOTH]
    # the tie: both ground truths of image 2 at IoU 0.3, the lower row is the argmax
    assert got["s"][dt_at[13], 0] == orclib.bb_iou([[0, 0, 10, 3]], [[0, 0, 10, 10]])[0, 0]
    assert got["arg"][dt_at[13], 0] == gt_at[6] < gt_at[7]
    # ... and the counts show it: the later one is held, the argmax is the missed one
    assert mg[dt_at[14], 0] == gt_at[7] - gt_at[6]
    assert got["hit"][0, gt_at[7]] and not got["hit"][0, gt_at[6]]


@pytest.fixture(scope="module", params=FIXTURES)
def golden(request):
    """(flat, restatement at IoU 0.5 and at 0.75 with the Python oracle's
    matches, recall of eval.npz, num_gt of the C oracle, categories to skip)."""
    from oracle import pyoracle
    from tao_amodal_amd import flatten as fl
    from tao_amodal_amd.columns import DTColumns, GTColumns
    name = request.param
    gtj, predj = load_inputs(name)
    f = fl.flatten_lvis(GTColumns.from_json(gtj), DTColumns.from_json(predj))
    res = pyoracle.lvis_eval(gtj, predj)
    n_dt = int(f.cell_dt_off[-1])
    mg = -np.ones((n_dt, 60), dtype=np.int32)
    for k in range(f.n_cells):
        d0, d1 = f.cell_dt_off[k], f.cell_dt_off[k + 1]
        g0, g1 = f.cell_gt_off[k], f.cell_gt_off[k + 1]
        if d1 == d0:
            continue
        cell = res["cells"][int(f.img_ids[f.cell_unit[k]]), int(f.cat_ids[f.cell_cat[k]])]
        gid = np.asarray(f.gt_id[g0:g1]).tolist()
        for a, e in enumerate(cell["ranges"]):
            assert e["dt_ids"] == np.asarray(f.dt_id[d0:d1]).tolist()
            for t in range(10):
                for j, v in enumerate(e["dt_matches"][t]):
                    if v != 0:
                        mg[d0 + j, a * 10 + t] = gid.index(int(v))
    gt_rng, _ = orclib.ranges(f)
    thrs, _ = orclib.thresholds()
    hidden = np.zeros(len(f.cat_ids), bool)
    hidden[np.asarray(f.gt_cat)[(np.asarray(f.gt_flags) & GT_ID_HIDDEN) != 0]] = True
    out = {t: ref.error_types(f, mg, gt_rng, thrs, t, 0.1) for t in (0, 5)}
    return f, out, load_eval(name)["lvis"][1], orclib.run_flat(f)["num_gt"], hidden, gt_rng


def test_fixture_codes_partition_the_rows(golden):
    f, out, _, _, _, _ = golden
    rows = np.bincount(np.asarray(f.dt_cat), minlength=len(f.cat_ids))
    for e in out.values():
        assert e["dt_type"].max(initial=0) <= 6
        assert np.array_equal(e["dt_counts"].sum(2), np.broadcast_to(rows, (6, len(rows))))


def test_fixture_counts_against_the_recorded_recall(golden):
    f, out, recall, num_gt, hidden, _ = golden
    keep = ~hidden
    for t, e in out.items():
        ev, missed = e["gt_counts"][..., 0], e["gt_counts"][..., 1]
        assert np.array_equal(ev.T, num_gt)
        tp = e["dt_counts"][..., ref.TP]
        want = np.where(num_gt > 0, np.round(recall[t] * num_gt), 0).astype(np.int64)
        assert np.array_equal(tp.T[keep], want[keep])
        assert np.array_equal(missed[:, keep], (ev - tp)[:, keep])
        assert (e["gt_counts"][..., 2] <= missed).all()


def test_fixture_every_dup_points_at_a_held_ground_truth(golden):
    """(Categories with a hidden-id ground truth aside: the Python oracle reports
    the detection such a ground truth holds as unmatched.)"""
    f, out, _, _, hidden, _ = golden
    for e in out.values():
        for a in range(6):
            dup = np.flatnonzero((e["dt_type"][:, a] == ref.DUP) & ~hidden[np.asarray(f.dt_cat)])
            assert (e["arg"][dup, a] >= 0).all()
            assert e["hit"][a, e["arg"][dup, a]].all()


def test_error_types_wants_evaluate_first_and_refuses_a_multi_gpu_run():
    from tao_amodal_amd.evaluation._dist import DistRun
    from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
    ev = LVISEval.__new__(LVISEval)
    ev._run = None
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.error_types()
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.error_lines()
    with pytest.raises(NotImplementedError, match=r"error_types\(\) in a multi-GPU run"):
        DistRun.__new__(DistRun).error_table(0, 0.1)


def test_abi_symbols_are_declared_exported_and_bound():
    from tao_amodal_amd import _lib
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    assert "#define TAOAMD_ERROR_TYPES_TILE %d" % _lib.ERROR_TYPES_TILE in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in ("taoamd_error_types_workspace", "taoamd_error_types"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.taoamd_version() >= 102
    assert _lib.ERROR_TYPES == ref.TYPES
    # sizes: one layout function, the types [n_dt][n_rng] and two byte tables [n_rng][n_gt]
    assert lib.taoamd_error_types_workspace(0, 0, 6) > 0
    small = lib.taoamd_error_types_workspace(1000, 1000, 1)
    assert small < lib.taoamd_error_types_workspace(1000, 1000, 6) \
        < lib.taoamd_error_types_workspace(1000, 100000, 6) \
        < lib.taoamd_error_types_workspace(100000, 100000, 6)
    assert lib.taoamd_error_types_workspace(1000, 1000, 9) == 0
    # refusals come before any launch
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    need = lib.taoamd_error_types_workspace(8, 8, 6)

    def call(n_rng=6, slot=0, tb=0.1, nbytes=need):
        return lib.taoamd_error_types(8, 8, 1, 3, n_rng, slot, tb, p, p, p, p, p, 60, p, p, p,
                                      p, p, p, p, p, p, None, p, nbytes, None)
    assert call(nbytes=need - 1) == 4
    for bad in (dict(slot=-1), dict(slot=10), dict(tb=0.5), dict(tb=0.75), dict(tb=-0.01),
                dict(tb=float("nan")), dict(n_rng=9), dict(n_rng=0)):
        assert call(**bad) == 2, bad
    assert call(slot=9, tb=0.94, nbytes=need - 1) == 4      # tf of slot 9 is 0.95
    assert call(slot=9, tb=0.95) == 2
