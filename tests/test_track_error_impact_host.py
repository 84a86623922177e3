"""The track-level error impact without a GPU: the numpy restatement
(tests/track_error_impact_ref.py) on the hand-written track table with the
links, the held marks, num_gt and precisions written out by hand, its BASE
against the C oracle's accumulate on the track side of the recorded fixtures,
and the C ABI's new symbols and the class methods."""
import os
import re

import numpy as np
import pytest

import orclib
import track_error_impact_ref as ref
import track_error_types_ref as te
from goldenio import load_inputs
from test_error_impact_host import expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["f1", "f2", "f3", "f4", "f5", "f7", "f9", "f10", "f11"]
# the fixtures with a ground-truth track whose id is hidden; on every other one
# BASE is the oracle's accumulate in every category
HIDDEN_IDS = ("f2", "f9")
GT_ID_HIDDEN = 4
N_RNG = 20


@pytest.fixture(scope="module")
def hand():
    f, dt_at, gt_at = te.hand_flat()
    gt_rng, dt_rng = orclib.ranges(f)
    iou, _ = orclib.track_iou(f)
    _, _, mg, _ = orclib.match(f, gt_rng, dt_rng, iou)
    thrs, rec = orclib.thresholds()
    out = ref.error_impact(f, iou, mg, gt_rng, dt_rng, thrs, 0, te.HAND_TB)
    return f, dt_at, gt_at, out, rec


def test_hand_written_table_links_held_and_num_gt(hand):
    f, dt_at, gt_at, out, _ = hand
    assert out["types"]["dt_type"][dt_at, 0].tolist() == te.HAND_TYPES_RNG0
    same, other, held = out["link_same"], out["link_other"], out["held"]
    # the LOC tracks 3, 9, 13, 15 of slot 0: the ground truth each overlaps best;
    # 13 ties between gt 6 and gt 7 and takes the lower row
    assert same[dt_at[[3, 9, 13, 15]], 0].tolist() == gt_at[[2, 5, 6, 8]].tolist()
    assert gt_at[6] < gt_at[7]
    # slot 1 ignores the long gt 8: track 15 links nothing there; slot 3 evaluates
    # gt 8 alone, and tracks 15 and 16, IGNORED there by their length, still link it
    assert same[dt_at[[15, 16]], 1].tolist() == [-1, -1]
    assert same[dt_at[[15, 16]], 3].tolist() == gt_at[[8, 8]].tolist()
    assert (same[dt_at[:15], 3] == -1).all() and (other[:, 3] == -1).all()
    # the CLS tracks 4 and 10, and the BOTH tracks 5 and 11
    assert other[dt_at[[4, 10, 5, 11]], 0].tolist() == gt_at[[3, 4, 3, 5]].tolist()
    # whatever the type: the TP track 0 links gt 3 of category 1
    assert other[dt_at[0], 0] == gt_at[3] and same[dt_at[0], 0] == gt_at[0]
    # an IoU of 0 is an overlap where nothing better exists: track 12 of category 2
    # shares no frame's area with gt 4 and gt 5, and links the lower row
    assert other[dt_at[12], 0] == gt_at[4] and same[dt_at[12], 0] == -1
    # gt 9 is ignored in every range: track 16 (IoU 1 with it) links nothing
    assert (other[dt_at[16]] == -1).all()
    # video 2 holds category 0 alone
    assert (other[dt_at[[13, 14]]] == -1).all()
    # held: the complement of missed among the evaluated (gt 1 is ignored, and held)
    assert held[0, gt_at].tolist() == [True, True, False, False, True, False, False, True,
                                      False, False]
    ev = ((np.asarray(out["types"]["gt_counts"])[0, :, 0]), out["types"]["gt_counts"][0, :, 1])
    assert ev[0].tolist() == [7, 1, 0] and ev[1].tolist() == [4, 1, 0]
    gt_rng = orclib.ranges(f)[0]
    for a in (0, 1, 3):
        open_ = ((gt_rng >> np.uint32(a)) & 1) == 0
        missed = np.bincount(np.asarray(f.gt_cat)[open_ & ~held[a]], minlength=3)
        assert missed.tolist() == out["types"]["gt_counts"][a, :, 1].tolist()
    # the nine num_gt: slot 0 (all, all), 1 (all, short), 3 (all, long)
    NG = out["num_gt"]
    for v in range(8):
        if v != ref.F_MISS:
            assert NG[v, :, [0, 1, 3]].tolist() == [[7, 1, 0], [6, 1, 0], [1, 0, 0]], v
    # every missed ground truth of slots 0 and 1 is linked; gt 8 in slot 3 is not:
    # its only neighbours there are IGNORED
    assert NG[ref.F_MISS, :, [0, 1, 3]].tolist() == [[7, 1, 0], [6, 1, 0], [0, 0, 0]]
    assert NG[ref.F_FN, :, [0, 1, 3]].tolist() == [[3, 0, 0], [3, 0, 0], [0, 0, 0]]
    # area 100: "small" (slots 4 .. 7) = "all"; nothing in the other area ranges
    assert np.array_equal(out["precision"][..., 4:8], out["precision"][..., 0:4])
    assert (out["precision"][..., 8:] == -1).all()
    assert out["events"]["adopted"] == 6          # gt 3's CLS track, in slots 0 .. 2 and 4 .. 6


def test_hand_written_table_precisions_as_fractions(hand):
    _, _, _, out, rec = hand
    P = out["precision"][..., 0]                        # [fix, R, category]

    def same(fix, cat, num_gt, by_count):
        assert np.array_equal(P[fix, :, cat], expected(num_gt, by_count, rec)), (fix, cat)

    def flat(tp, n, upto):
        return {c: (tp, n) for c in range(upto + 1)}
    # category 0 by score: T .95 | T T LOC LOC .9 | DUP BKG .8 (the IGNORED row is
    # dropped) | DUP LOC .7 | LOC .6 | CLS .5 | BOTH .4 | BKG .3
    same(ref.BASE, 0, 7, flat(3, 3, 3))
    # LOC: each of the four LOC tracks is the only one linking its missed ground truth
    same(ref.F_LOC, 0, 7, {**flat(5, 5, 5), 6: (7, 10), 7: (7, 10)})
    for fix in (ref.F_CLS, ref.F_BOTH, ref.F_DUP, ref.F_BKG, ref.F_MISS, ref.F_FP):
        same(fix, 0, 7, flat(3, 3, 3))
    same(ref.F_FN, 0, 3, flat(3, 3, 3))
    # category 1: CLS .6 (its link gt 4 is held: it just leaves), BOTH .5; track 4
    # of category 0 (score 0.5) is adopted BEHIND the BOTH row of the same score
    same(ref.BASE, 1, 1, {})
    same(ref.F_CLS, 1, 1, flat(1, 2, 1))
    same(ref.F_LOC, 1, 1, {})
    assert (P[ref.F_FN, :, 1] == -1).all() and (P[:, :, 2] == -1).all()
    # slot 3 (long): gt 8 alone, no row is kept; MISS and FN empty the category
    P3 = out["precision"][..., 3]
    assert (P3[[ref.BASE, ref.F_LOC, ref.F_FP], :, 0] == 0).all()
    assert (P3[[ref.F_MISS, ref.F_FN], :, 0] == -1).all()


def test_rows_the_lists_leave_out_link_nothing(hand):
    f, dt_at, gt_at, out, _ = hand
    gt_rng = orclib.ranges(f)[0]
    gl = np.ones(len(f.gt_cat), bool)
    gl[gt_at[3]] = False
    dl = np.ones(len(f.dt_cat), bool)
    dl[dt_at[10]] = False
    got = ref.other_links(f, gt_rng, N_RNG, dt_listed=dl, gt_listed=gl)
    assert (got[dt_at[[4, 5, 10]]] == -1).all() and got[dt_at[11], 0] == gt_at[5]
    assert np.array_equal(ref.other_links(f, gt_rng, N_RNG), out["link_other"])


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_base_is_the_oracles_accumulate(name):
    from tao_amodal_amd import engine, flatten as fl
    from tao_amodal_amd.columns import DTColumns, GTColumns
    gtj, predj = load_inputs(name)
    dt = DTColumns.from_json(predj)
    dt.track_id, _ = fl.make_track_ids_unique(dt)
    f = fl.flatten_tao(GTColumns.from_json(gtj), dt)
    iou, _ = orclib.track_iou(f)
    if name == "f7":
        # (the matrix the guarded pass holds: see test_track_error_types_host.golden)
        iou = engine.set_order_iou(f, np.arange(len(iou)))
    gt_rng, dt_rng = orclib.ranges(f)
    matched, ignored, mg, _ = orclib.match(f, gt_rng, dt_rng, iou)
    precision, _, _, num_gt = orclib.accumulate(f, gt_rng, matched, ignored)
    thrs, _ = orclib.thresholds()
    hidden = np.zeros(len(f.cat_ids), bool)
    hidden[np.asarray(f.gt_cat)[(np.asarray(f.gt_flags) & GT_ID_HIDDEN) != 0]] = True
    # the cap on what is set aside: nothing, but on the two fixtures with hidden
    # ids (f9: one category, a hidden id in it; f2: one of eight)
    assert hidden.any() == (name in HIDDEN_IDS)
    assert name != "f2" or hidden.sum() == 1
    for t in (0, 5):
        out = ref.error_impact(f, iou, mg, gt_rng, dt_rng, thrs, t, 0.1)
        assert np.array_equal(out["precision"][ref.BASE][:, ~hidden], precision[t][:, ~hidden])
        assert np.array_equal(out["num_gt"][ref.BASE], num_gt)
        # a fix of false positives or of misses never lowers a precision value
        for v in (ref.F_BOTH, ref.F_DUP, ref.F_BKG, ref.F_FP, ref.F_MISS, ref.F_FN):
            live = out["precision"][v] >= 0
            assert (out["precision"][v][live] >= out["precision"][ref.BASE][live]).all()


def test_abi_symbols_are_declared_exported_and_bound():
    from tao_amodal_amd import _lib
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in ("taoamd_track_error_types_links", "taoamd_track_error_impact_workspace",
                 "taoamd_track_error_impact"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.taoamd_version() >= 106
    size = lib.taoamd_track_error_impact_workspace
    assert size(0, 0, 1, 20) > 0
    assert size(1000, 1000, 5, 1) < size(1000, 1000, 5, 9) < size(1000, 1000, 5, 20) \
        < size(1000, 100000, 5, 20) < size(100000, 100000, 5, 20)
    assert size(1000, 1000, 5, 21) == 0 and size(1000, 1000, 5, 0) == 0 \
        and size(1000, 1000, 0, 20) == 0
    # the same function of its sizes as the image level's, which keeps its limit
    assert size(1000, 1000, 5, 8) == lib.taoamd_error_impact_workspace(1000, 1000, 5, 8)
    assert lib.taoamd_error_impact_workspace(1000, 1000, 5, 9) == 0
    # refusals come before any launch
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    need = size(8, 8, 3, 20)
    assert need <= buf.nbytes

    def sweep(entry="taoamd_track_error_impact", n_rng=20, n_cat=3, nbytes=need, held=p):
        return getattr(lib, entry)(8, 8, n_cat, n_rng, p, p, p, p, p, p, p, p, p, held, p, p, p,
                                   nbytes, None)
    assert sweep(nbytes=need - 1) == 4
    for bad in (dict(n_rng=0), dict(n_rng=21), dict(n_cat=0), dict(held=None)):
        assert sweep(**bad) == 2, bad
    assert sweep("taoamd_error_impact", n_rng=9) == 2
    # the links entry: the three tables are required
    need = lib.taoamd_track_error_types_workspace(8, 8, 20)

    def links(n_rng=20, slot=0, tb=0.1, nbytes=need, same=p, other=p, held=p):
        return lib.taoamd_track_error_types_links(
            8, 8, 1, 8, 1, 3, n_rng, slot, tb, p, p, p, p, p, p, 200, p, p, p, p, p, p, p, p,
            p, p, p, p, p, p, None, None, same, other, held, p, nbytes, None)
    for bad in (dict(same=None), dict(other=None), dict(held=None), dict(slot=10),
                dict(tb=0.5), dict(n_rng=21), dict(n_rng=0)):
        assert links(**bad) == 2, bad
    assert links(nbytes=need - 1) == 4


def test_error_impact_wants_evaluate_first():
    from tao_amodal_amd.evaluation.tao_amodal import TaoEval
    assert callable(TaoEval.error_impact) and callable(TaoEval.impact_lines)
    ev = TaoEval.__new__(TaoEval)
    ev._run = None
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.error_impact()
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.impact_lines()
