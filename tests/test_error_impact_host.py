"""The error impact without a GPU: the numpy restatement
(tests/error_impact_ref.py) on a hand-written table with the expected
precisions written out as fractions, its BASE against the C oracle's accumulate
on the recorded fixtures, and the C ABI's new symbols and refusals."""
import os
import re

import numpy as np
import pytest

import error_impact_ref as ref
import error_types_ref as et
import orclib
from goldenio import load_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["f1", "f2", "f3", "f4", "f5", "f7", "f9", "f10"]
GT_ID_HIDDEN = 4
NAN = float("nan")

# ---------------------------------------------------------------------------
# HAND_* of error_types_ref (images 0-2, categories 0-2) and, in images and
# categories of their own, the cases of the fixes.  tf = 0.5, tb = 0.125; every
# ground truth is fully visible: ranges 0 and 3 evaluate it.
# ---------------------------------------------------------------------------
GTS = et.HAND_GTS + [
    # image 3, category 3: the LOC fix
    (3, 3, [0, 0, 10, 10], 1.0, 0),      # 8  gA missed: two LOC rows, scores 0.7 and 0.5
    (3, 3, [100, 0, 10, 10], 1.0, 0),    # 9  gB missed: two LOC rows of score 0.6
    (3, 3, [200, 0, 10, 10], 1.0, 0),    # 10 gC missed: LOC rows of score 0.1 and NaN
    (3, 3, [300, 0, 10, 10], 1.0, 0),    # 11 gD held, and linked by a LOC row
    (3, 3, [400, 0, 10, 10], 1.0, 0),    # 12 gJ missed, nothing links it
    # image 4, category 4: the CLS fix
    (4, 4, [0, 0, 10, 10], 1.0, 0),      # 13 gE missed: CLS rows of categories 5 (0.3) and 6 (0.9)
    (4, 4, [100, 0, 10, 10], 1.0, 0),    # 14 gF missed: CLS rows of categories 5 (NaN) and 6 (0.2)
    # image 5: a true positive each for categories 5 and 6
    (5, 5, [0, 0, 10, 10], 1.0, 0),      # 15 gG
    (5, 6, [100, 0, 10, 10], 1.0, 0),    # 16 gH
    # category 7: emptied by MISS
    (6, 7, [0, 0, 10, 10], 1.0, 0),      # 17 gI missed, unlinked
    (7, 7, [300, 0, 10, 10], 1.0, 0),    # 18 gL missed, near a BOTH row only: unlinked
    (7, 8, [0, 0, 10, 10], 1.0, 0),      # 19 gK held
]
DETS = et.HAND_DETS + [
    (3, 3, [300, 0, 10, 10], 0.8, 0),    # 15 TP on gD
    (3, 3, [300, 0, 10, 3], 0.75, 0),    # 16 LOC, link held: leaves
    (3, 3, [0, 0, 10, 3], 0.7, 0),       # 17 LOC -> gA: the winner
    (3, 3, [100, 0, 10, 3], 0.6, 0),     # 18 LOC -> gB: the winner, the lower row
    (3, 3, [100, 0, 10, 3], 0.6, 0),     # 19 LOC -> gB: leaves
    (3, 3, [0, 0, 10, 3], 0.5, 0),       # 20 LOC -> gA: leaves
    (3, 3, [200, 0, 10, 3], 0.1, 0),     # 21 LOC -> gC: the winner
    (3, 3, [200, 0, 10, 3], NAN, 0),     # 22 LOC -> gC: leaves
    (4, 4, [500, 500, 5, 5], 0.9, 0),    # 23-28 BKG rows of category 4
    (4, 4, [500, 500, 5, 5], 0.9, 0),
    (4, 4, [500, 500, 5, 5], 0.5, 0),
    (4, 4, [500, 500, 5, 5], 0.4, 0),
    (4, 4, [500, 500, 5, 5], 0.3, 0),
    (4, 4, [500, 500, 5, 5], 0.25, 0),
    (4, 5, [0, 0, 10, 10], 0.3, 0),      # 29 CLS -> gE: the lower row, the lower score: loses
    (4, 5, [100, 0, 10, 10], NAN, 0),    # 30 CLS -> gF: a NaN loses to a number in a higher row
    (4, 6, [0, 0, 10, 10], 0.9, 0),      # 31 CLS -> gE: adopted by category 4 behind its 0.9 rows
    (4, 6, [100, 0, 10, 10], 0.2, 0),    # 32 CLS -> gF: adopted at the end
    (5, 5, [0, 0, 10, 10], 0.1, 0),      # 33 TP on gG
    (5, 6, [100, 0, 10, 10], 0.5, 0),    # 34 TP on gH
    (6, 7, [500, 500, 5, 5], 0.5, 0),    # 35 BKG
    (7, 8, [500, 500, 5, 5], 0.9, 0),    # 36 BKG
    (7, 8, [300, 0, 10, 2], 0.8, 0),     # 37 BOTH: IoU 0.2 with gL of category 7
    (7, 8, [0, 0, 10, 10], 0.7, 0),      # 38 TP on gK
    (7, 8, [0, 0, 10, 9], 0.6, 0),       # 39 DUP
]
NEW_TYPES_RNG0 = [0, 3, 3, 3, 3, 3, 3, 3, 6, 6, 6, 6, 6, 6, 4, 4, 4, 4, 0, 0, 6, 6, 5, 0, 2]
N_IMG, N_CAT = 8, 9


def expected(num_gt, by_count, rec_thrs):
    """precision[R] from {c: (tp, n)}: the fraction at every threshold whose
    recall is first reached at true-positive count c; counts not named: 0."""
    out = np.zeros(len(rec_thrs))
    counts = np.arange(num_gt + 1)
    for j, thr in enumerate(rec_thrs):
        c = int(np.searchsorted(counts / num_gt, thr, side="left"))
        if c in by_count:
            tp, n = by_count[c]
            out[j] = tp / (n + np.spacing(1))
    return out


@pytest.fixture(scope="module")
def hand():
    f, dt_at, gt_at = et.make_flat(N_IMG, N_CAT, DETS, GTS)
    gt_rng, dt_rng = orclib.ranges(f)
    _, _, mg, _ = orclib.match(f, gt_rng, dt_rng)
    thrs, rec = orclib.thresholds()
    out = ref.error_impact(f, mg, gt_rng, thrs, 0, et.HAND_TB)
    return f, dt_at, gt_at, out, rec


def test_hand_written_table_types_links_and_events(hand):
    f, dt_at, gt_at, out, _ = hand
    ty = out["types"]["dt_type"]
    assert ty[dt_at, 0].tolist() == et.HAND_TYPES_RNG0 + NEW_TYPES_RNG0
    # links: whatever the row's type
    assert out["link_same"][dt_at[[16, 17, 20]], 0].tolist() == gt_at[[11, 8, 8]].tolist()
    assert out["link_other"][dt_at[[29, 31, 30, 32, 4, 10]], 0].tolist() == \
        gt_at[[13, 13, 14, 14, 3, 4]].tolist()
    assert out["link_other"][dt_at[0], 0] == gt_at[3]        # a TP row has links too
    # (an IoU of 0 is an overlap like any other: the first ground truth of the category)
    assert out["link_same"][dt_at[35], 0] == gt_at[17] and out["link_other"][dt_at[35], 0] == -1
    assert out["link_same"][dt_at[12], 0] == -1 and out["link_other"][dt_at[12], 0] == gt_at[4]
    assert out["held"][0, gt_at[[11, 15, 16, 19]]].all()
    assert not out["held"][0, gt_at[[8, 9, 10, 12, 13, 14, 17, 18]]].any()
    # ranges 0 and 3 only; per range: winners gt 2, 5, 6, gA, gB, gC (LOC), gt 3, gE,
    # gF (CLS); d10 and d16 link held ground truths; d19, d20, d22, d29, d30 lose
    assert out["events"] == dict(winner=18, lost_to_held=4, lost_to_better=10, adopted=6,
                                 unlinked_missed=6, linked_missed=18)
    assert out["num_gt"][ref.BASE, :, 0].tolist() == [6, 1, 0, 5, 2, 1, 1, 2, 1]
    assert out["num_gt"][ref.F_MISS, :, 0].tolist() == [6, 1, 0, 4, 2, 1, 1, 0, 1]
    assert out["num_gt"][ref.F_FN, :, 0].tolist() == [3, 0, 0, 1, 0, 1, 1, 0, 1]
    for v in (ref.F_CLS, ref.F_LOC, ref.F_BOTH, ref.F_DUP, ref.F_BKG, ref.F_FP):
        assert np.array_equal(out["num_gt"][v], out["num_gt"][ref.BASE])
    assert np.array_equal(out["precision"][..., 3], out["precision"][..., 0])
    assert (out["precision"][..., [1, 2, 4, 5]] == -1).all()


def test_hand_written_table_precisions_as_fractions(hand):
    _, _, _, out, rec = hand
    P = out["precision"][..., 0]                        # [fix, R, category]

    def same(fix, cat, num_gt, by_count):
        assert np.array_equal(P[fix, :, cat], expected(num_gt, by_count, rec)), (fix, cat)

    def flat(tp, n, upto):
        return {c: (tp, n) for c in range(upto + 1)}
    # category 0, by score: T T T | LOC .9 | DUP .8 DUP .7 | LOC .7 LOC .6 | CLS BOTH BKG
    same(ref.BASE, 0, 6, flat(3, 3, 3))
    same(ref.F_LOC, 0, 6, {**flat(4, 4, 4), 5: (6, 8), 6: (6, 8)})
    for fix in (ref.F_CLS, ref.F_BOTH, ref.F_DUP, ref.F_BKG, ref.F_MISS, ref.F_FP):
        same(fix, 0, 6, flat(3, 3, 3))
    same(ref.F_FN, 0, 3, flat(3, 3, 3))
    # category 1: CLS .6 (its link is held: it just leaves), BOTH .5; d4 of
    # category 0 (score 0.5) is adopted BEHIND the BOTH row of the same score
    same(ref.BASE, 1, 1, {})
    same(ref.F_CLS, 1, 1, flat(1, 2, 1))
    assert (P[ref.F_FN, :, 1] == -1).all() and (P[:, :, 2] == -1).all()
    # category 3: TP .8, then seven LOC rows; one links a held ground truth, three win
    same(ref.BASE, 3, 5, flat(1, 1, 1))
    same(ref.F_LOC, 3, 5, flat(4, 4, 4))
    same(ref.F_MISS, 3, 4, flat(1, 1, 1))
    same(ref.F_FN, 3, 1, flat(1, 1, 1))
    same(ref.F_FP, 3, 5, flat(1, 1, 1))
    # category 4: F .9 F .9 [T .9] F .5 F .4 F .3 F .25 [T .2]
    same(ref.BASE, 4, 2, {})
    same(ref.F_CLS, 4, 2, {0: (1, 3), 1: (1, 3), 2: (2, 8)})
    assert (P[ref.F_FN, :, 4] == -1).all()
    # categories 5 and 6: a CLS row above the true positive
    for cat in (5, 6):
        same(ref.BASE, cat, 1, flat(1, 2, 1))
        same(ref.F_CLS, cat, 1, flat(1, 1, 1))
        same(ref.F_FP, cat, 1, flat(1, 1, 1))
    # category 7: emptied by MISS
    same(ref.BASE, 7, 2, {})
    assert (P[ref.F_MISS, :, 7] == -1).all() and (P[ref.F_FN, :, 7] == -1).all()
    # category 8: BKG .9, BOTH .8, TP .7, DUP .6
    same(ref.BASE, 8, 1, flat(1, 3, 1))
    same(ref.F_BKG, 8, 1, flat(1, 2, 1))
    same(ref.F_BOTH, 8, 1, flat(1, 2, 1))
    same(ref.F_DUP, 8, 1, flat(1, 3, 1))
    same(ref.F_FP, 8, 1, flat(1, 1, 1))


def test_winner_rule():
    assert ref.better(0.5, 0.4) and not ref.better(0.4, 0.5)
    assert not ref.better(0.0, -0.0) and not ref.better(-0.0, 0.0)      # the lower row keeps it
    assert ref.better(-1e300, NAN) and not ref.better(NAN, -1e300) and not ref.better(NAN, NAN)
    assert ref.better(float("-inf"), NAN) and not ref.better(0.3, 0.3)


def test_adopted_rows_go_behind_equal_scores_and_nan_to_the_end():
    """impact_tables on a bare table: category 0 holds F .5, F .5, F NaN; two CLS
    rows of category 1 (scores .5 and NaN) are adopted for two missed ground truths."""
    rec = orclib.thresholds()[1]
    dt_cat = [0, 0, 0, 1, 1]
    score = [0.5, 0.5, NAN, 0.5, NAN]
    ty = np.array([[et.BKG], [et.BKG], [et.BKG], [et.CLS], [et.CLS]], dtype=np.uint8)
    none = -np.ones((5, 1), dtype=np.int64)
    other = none.copy()
    other[3, 0], other[4, 0] = 0, 1
    out = ref.impact_tables(2, 1, dt_cat, score, ty, none, other, [0, 0], [0, 0],
                            np.zeros((1, 2), bool), rec)
    # F F [T .5] F(NaN) [T NaN]
    want = expected(2, {0: (2, 5), 1: (2, 5), 2: (2, 5)}, rec)
    assert np.array_equal(out["precision"][ref.F_CLS, :, 0, 0], want)
    assert 2 / (5 + np.spacing(1)) > 1 / (3 + np.spacing(1))
    assert out["events"]["adopted"] == 2


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_base_is_the_oracles_accumulate(name):
    from tao_amodal_amd import flatten as fl
    from tao_amodal_amd.columns import DTColumns, GTColumns
    gtj, predj = load_inputs(name)
    f = fl.flatten_lvis(GTColumns.from_json(gtj), DTColumns.from_json(predj))
    r = orclib.run_flat(f)
    thrs, _ = orclib.thresholds()
    hidden = np.zeros(len(f.cat_ids), bool)
    hidden[np.asarray(f.gt_cat)[(np.asarray(f.gt_flags) & GT_ID_HIDDEN) != 0]] = True
    assert name == "f9" or not hidden.all()      # (f9: one category, a hidden id in it)
    for t in (0, 5):
        out = ref.error_impact(f, r["match_gt"], r["gt_rng"], thrs, t, 0.1)
        assert np.array_equal(out["precision"][ref.BASE][:, ~hidden], r["precision"][t][:, ~hidden])
        assert np.array_equal(out["num_gt"][ref.BASE], r["num_gt"])
        # a fix of false positives or of misses never lowers a precision value
        for v in (ref.F_BOTH, ref.F_DUP, ref.F_BKG, ref.F_FP, ref.F_MISS, ref.F_FN):
            live = out["precision"][v] >= 0
            assert (out["precision"][v][live] >= out["precision"][ref.BASE][live]).all()


def test_abi_symbols_are_declared_exported_and_bound():
    from tao_amodal_amd import _lib
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    assert "#define TAOAMD_ERROR_IMPACT_CHUNK %d" % _lib.ERROR_IMPACT_CHUNK in text
    assert "#define TAOAMD_ERROR_IMPACT_FIXES %d" % len(_lib.ERROR_FIXES) in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in ("taoamd_error_types_links", "taoamd_error_impact_workspace",
                 "taoamd_error_impact"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.taoamd_version() >= 105
    assert _lib.ERROR_FIXES == ref.FIXES
    size = lib.taoamd_error_impact_workspace
    assert size(0, 0, 1, 6) > 0
    assert size(1000, 1000, 5, 1) < size(1000, 1000, 5, 6) < size(1000, 100000, 5, 6) \
        < size(100000, 100000, 5, 6) <= size(100000, 100000, 5000, 6)
    assert size(1000, 1000, 5, 9) == 0 and size(1000, 1000, 0, 6) == 0
    # refusals come before any launch
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    need = size(8, 8, 3, 6)
    assert need <= buf.nbytes

    def call(n_rng=6, n_cat=3, nbytes=need, held=p):
        return lib.taoamd_error_impact(8, 8, n_cat, n_rng, p, p, p, p, p, p, p, p, p, held, p, p,
                                       p, nbytes, None)
    assert call(nbytes=need - 1) == 4
    for bad in (dict(n_rng=0), dict(n_rng=9), dict(n_cat=0), dict(held=None)):
        assert call(**bad) == 2, bad
    # the links entry: the three tables are required
    need = lib.taoamd_error_types_workspace(8, 8, 6)

    def links(slot=0, tb=0.1, nbytes=need, link=p):
        return lib.taoamd_error_types_links(8, 8, 1, 3, 6, slot, tb, p, p, p, p, p, 60, p, p, p,
                                            p, p, p, p, p, p, None, link, p, p, p, nbytes, None)
    assert links(link=None) == 2 and links(slot=10) == 2 and links(tb=0.5) == 2
    assert links(nbytes=need - 1) == 4
