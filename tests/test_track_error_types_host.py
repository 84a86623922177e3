"""The track-level error breakdown without a GPU: the numpy restatement
(tests/track_error_types_ref.py) on a hand-written track table with literal
expectations, on the track side of the recorded fixtures with the C oracle's
matches, and the C ABI's new symbols and refusals."""
import os
import re

import numpy as np
import pytest

import orclib
import track_error_types_ref as ref
from goldenio import load_eval, load_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["f1", "f2", "f3", "f4", "f5", "f7", "f9", "f10", "f11"]
GT_ID_HIDDEN = 4
DT_NO_CONSUME = 2
N_RNG = 20


def _oracle_tables(f, iou=None):
    gt_rng, dt_rng = orclib.ranges(f)
    if iou is None:
        iou, _ = orclib.track_iou(f)
    _, _, mg, _ = orclib.match(f, gt_rng, dt_rng, iou)
    return iou, gt_rng, dt_rng, mg


def test_hand_written_table_one_detection_track_of_each_type():
    f, dt_at, gt_at = ref.hand_flat()
    iou, gt_rng, dt_rng, mg = _oracle_tables(f)
    thrs, _ = orclib.thresholds()
    assert thrs[0] == 0.5
    # the pinned IoUs are exact in the oracle's arithmetic
    def row(d):          # the row of detection track d in its cell's IoU matrix
        k = f.dt_cell[d]
        G = f.cell_gt_off[k + 1] - f.cell_gt_off[k]
        at = f.cell_iou_off[k] + (d - f.cell_dt_off[k]) * G
        return iou[at:at + G].tolist()
    assert row(dt_at[7]) == [0.5, 0.0] and row(dt_at[9]) == [0.0, 0.125]
    got = ref.error_types(f, iou, mg, gt_rng, dt_rng, thrs, 0, ref.HAND_TB)
    assert got["dt_type"][dt_at, 0].tolist() == ref.HAND_TYPES_RNG0
    assert got["dt_type"][dt_at, 1].tolist() == ref.HAND_TYPES_RNG1
    assert got["dt_type"][dt_at, 3].tolist() == ref.HAND_TYPES_RNG3
    assert got["dt_type"][dt_at[:7], 0].tolist() == list(range(7))   # video 0: each type once
    assert got["dt_counts"][0].tolist() == ref.HAND_DT_COUNTS_RNG0
    assert got["gt_counts"][0].tolist() == ref.HAND_GT_COUNTS_RNG0
    assert got["gt_counts"][3].tolist() == ref.HAND_GT_COUNTS_RNG3
    # area 100: "small" (slots 4 .. 7) = "all", nothing in "medium", "large"; no
    # ground truth has occluded frames, so the last area range evaluates none
    assert np.array_equal(got["dt_counts"][4:8], got["dt_counts"][0:4])
    assert not got["gt_counts"][8:].any()
    # the cross-category result alone
    for d in range(len(ref.HAND_DETS)):
        want = ref.HAND_OVER_RNG0.get(d, (0, 0))
        assert tuple(int(w) & 1 for w in got["dt_over"][dt_at[d]]) == want, d
    # ignored through dt_rng ONLY: track 15 carries no flag, its length does it
    assert f.dt_flags[dt_at[15]] == 0 and (dt_rng[dt_at[15]] >> 3) & 1 and not dt_rng[dt_at[15]] & 1
    # track 16 would be CLS (IoU 1) were gt 9 evaluated anywhere
    blocks = ref.cross_blocks(f)
    D, G, m = [b for b in blocks if dt_at[16] in b[0]][0]
    assert m[list(D).index(dt_at[16]), list(G).index(gt_at[9])] == 1.0
    assert gt_rng[gt_at[9]] == (1 << N_RNG) - 1
    # >= at both thresholds: just above either, the four pinned rows fall a class
    up = ref.error_types(f, iou, mg, gt_rng, dt_rng, thrs, 0, 0.125 + 2.0 ** -50)
    assert up["dt_type"][dt_at[[9, 11]], 0].tolist() == [ref.BKG, ref.BKG]
    assert up["gt_counts"][0, 0].tolist() == [7, 4, 3]
    thr_up = thrs.copy()
    thr_up[1] = 0.5 + 2.0 ** -50
    mg1 = mg.copy()
    mg1[:, 1::10] = mg[:, 0::10]
    mg1[dt_at[7], 1::10] = -1               # (IoU 0.5 is below it: no match)
    at = ref.error_types(f, iou, mg1, gt_rng, dt_rng, thr_up, 1, ref.HAND_TB)
    assert at["dt_type"][dt_at[[7, 8, 10]], 0].tolist() == [ref.LOC, ref.LOC, ref.BOTH]
    # the tie: both ground truths of video 2 at IoU 0.3, the lower row is the argmax
    assert got["s"][dt_at[13], 0] == orclib.bb_iou([[0, 0, 10, 3]], [[0, 0, 10, 10]])[0, 0]
    assert got["arg"][dt_at[13], 0] == gt_at[6] < gt_at[7]
    # ... and the counts show it: the later one is held, the argmax is the missed one
    assert mg[dt_at[14], 0] == gt_at[7] - gt_at[6]
    assert got["hit"][0, gt_at[7]] and not got["hit"][0, gt_at[6]]


def test_rows_the_lists_leave_out_have_no_cross_category_overlap():
    f, dt_at, gt_at = ref.hand_flat()
    iou, gt_rng, dt_rng, mg = _oracle_tables(f)
    thrs, _ = orclib.thresholds()
    gl = np.ones(len(f.gt_cat), bool)
    gl[gt_at[3]] = False
    dl = np.ones(len(f.dt_cat), bool)
    dl[dt_at[10]] = False
    got = ref.error_types(f, iou, mg, gt_rng, dt_rng, thrs, 0, ref.HAND_TB,
                          dt_listed=dl, gt_listed=gl)
    assert got["dt_type"][dt_at[[4, 5, 10, 11]], 0].tolist() == [ref.BKG, ref.BKG, ref.BKG, ref.BOTH]


@pytest.fixture(scope="module", params=FIXTURES)
def golden(request):
    """(flat, restatement at IoU 0.5 and 0.75 (bg 0.1) and at 0.5 with bg 0 with
    the C oracle's matches, recall of eval.npz, num_gt of the C oracle,
    categories with a hidden-id ground truth or a track that does not consume)."""
    from tao_amodal_amd import engine, flatten as fl
    from tao_amodal_amd.columns import DTColumns, GTColumns
    name = request.param
    gtj, predj = load_inputs(name)
    dt = DTColumns.from_json(predj)
    dt.track_id, _ = fl.make_track_ids_unique(dt)
    f = fl.flatten_tao(GTColumns.from_json(gtj), dt)
    iou, _ = orclib.track_iou(f)
    if name == "f7":
        # every IoU within ulps of a threshold: the recorded results are those of
        # the reference's set-order sums, the matrix the guarded pass holds
        iou = engine.set_order_iou(f, np.arange(len(iou)))
    iou, gt_rng, dt_rng, mg = _oracle_tables(f, iou)
    thrs, _ = orclib.thresholds()
    hidden = np.zeros(len(f.cat_ids), bool)
    hidden[np.asarray(f.gt_cat)[(np.asarray(f.gt_flags) & GT_ID_HIDDEN) != 0]] = True
    # (a track whose id is no positive number matches without consuming: its
    # ground truth may hold a second track, so TP counts tracks, not ground
    # truths, in its category -- f11's motif; set aside like the hidden ids)
    hidden[np.asarray(f.dt_cat)[(np.asarray(f.dt_flags) & DT_NO_CONSUME) != 0]] = True
    out = {(t, tb): ref.error_types(f, iou, mg, gt_rng, dt_rng, thrs, t, tb)
           for t, tb in ((0, 0.1), (5, 0.1), (0, 0.0))}
    num_gt = orclib.accumulate(f, gt_rng, *orclib.match(f, gt_rng, dt_rng, iou, False)[:2])[3]
    recall = load_eval(name)["tao"][1]
    return f, out, recall.reshape(recall.shape[0], recall.shape[1], -1), num_gt, hidden, dt_rng


def test_fixture_codes_partition_the_rows(golden):
    f, out, _, _, _, _ = golden
    rows = np.bincount(np.asarray(f.dt_cat), minlength=len(f.cat_ids))
    for e in out.values():
        assert e["dt_type"].max(initial=0) <= 6
        assert np.array_equal(e["dt_counts"].sum(2), np.broadcast_to(rows, (N_RNG, len(rows))))


def test_fixture_counts_against_the_recorded_recall(golden):
    f, out, recall, num_gt, hidden, _ = golden
    keep = ~hidden
    for (t, _), e in out.items():
        ev, missed = e["gt_counts"][..., 0], e["gt_counts"][..., 1]
        assert np.array_equal(ev.T, num_gt)
        tp = e["dt_counts"][..., ref.TP]
        want = np.where(num_gt > 0, np.round(recall[t] * num_gt), 0).astype(np.int64)
        assert np.array_equal(tp.T[keep], want[keep])
        assert np.array_equal(missed[:, keep], (ev - tp)[:, keep])
        assert (e["gt_counts"][..., 2] <= missed).all()


def test_fixture_every_dup_points_at_a_held_ground_truth(golden):
    f, out, _, _, _, _ = golden
    for e in out.values():
        for a in range(N_RNG):
            dup = np.flatnonzero(e["dt_type"][:, a] == ref.DUP)
            assert (e["arg"][dup, a] >= 0).all()
            assert e["hit"][a, e["arg"][dup, a]].all()


def test_fixture_with_no_background_threshold_every_open_row_is_dup_or_loc(golden):
    f, out, _, _, _, dt_rng = golden
    e = out[0, 0.0]
    for a in range(N_RNG):
        t = e["dt_type"][:, a]
        open_ = (t != ref.TP) & (t != ref.IGNORED)
        assert np.isin(t[open_], (ref.DUP, ref.LOC)).all()
        # IGNORED without a match is dt_rng's bit
        assert ((dt_rng >> np.uint32(a)) & 1)[open_].sum() == 0
    # ... and dt_over's word 1 is every range: the empty maximum is 0 >= 0
    assert (e["dt_over"][:, 1] == (1 << N_RNG) - 1).all()


def test_error_types_wants_evaluate_first_and_refuses_a_multi_gpu_run():
    from tao_amodal_amd.evaluation._dist import DistRun
    from tao_amodal_amd.evaluation.tao_amodal import TaoEval
    ev = TaoEval.__new__(TaoEval)
    ev._run = None
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.error_types()
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.error_lines()
    with pytest.raises(NotImplementedError, match=r"a video's"):
        DistRun.__new__(DistRun).error_table(0, 0.1)


def test_abi_symbols_are_declared_exported_and_bound():
    from tao_amodal_amd import _lib
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    assert "#define TAOAMD_TRACK_ERROR_TYPES_TILE %d" % _lib.TRACK_ERROR_TYPES_TILE in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in ("taoamd_track_error_types_workspace", "taoamd_track_error_types"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.taoamd_version() >= 103
    assert _lib.ERROR_TYPES == ref.TYPES
    # sizes: one layout function, two masks a row and two byte tables [n_rng][n_gt]
    size = lib.taoamd_track_error_types_workspace
    assert size(0, 0, 20) > 0
    assert size(1000, 1000, 1) < size(1000, 1000, 20) < size(1000, 100000, 20) \
        < size(100000, 100000, 20)
    assert size(1000, 1000, 21) == 0 and size(1000, 1000, 0) == 0
    # refusals come before any launch
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    need = size(8, 8, 20)

    def call(n_rng=20, slot=0, tb=0.1, nbytes=need):
        return lib.taoamd_track_error_types(
            8, 8, 1, 8, 1, 3, n_rng, slot, tb, p, p, p, p, p, p, 200, p, p, p, p, p, p, p, p,
            p, p, p, p, p, p, None, None, p, nbytes, None)
    assert call(nbytes=need - 1) == 4
    for bad in (dict(slot=-1), dict(slot=10), dict(tb=0.5), dict(tb=0.75), dict(tb=-0.01),
                dict(tb=float("nan")), dict(n_rng=21), dict(n_rng=0)):
        assert call(**bad) == 2, bad
    assert call(slot=9, tb=0.94, nbytes=need - 1) == 4      # tf of slot 9 is 0.95
    assert call(slot=9, tb=0.95) == 2
