"""Scores that are any double, on the host: the expectation the GPU tests of
test_gpu_score_values.py compare with is pinned here (numpy's order of NaN,
infinities, signed zeros and subnormals on a hand-written vector), and so are
the populations, the host sorter, flatten.py's cut at max_dets against
pyoracle's, the track mean of long tracks against np.mean, and the C oracle's
order against numpy's."""
import numpy as np
import pytest

import orclib
import scorepop
from oracle import pyoracle
from scorepop import KINDS, NAN_BITS, bits, expected_order, score_population
from tao_amodal_amd import flatten as fl


def test_numpy_puts_every_nan_last_in_input_order():
    """The expectation itself: np.argsort(-score, kind="mergesort") == lexsort
    with the index as the last key; -0.0 ties with 0.0, 5e-324 lies above
    them, every NaN is last whatever its sign bit or payload."""
    neg_nan = np.array([0xfff8000000000001], np.uint64).view(np.float64)[0]
    s = np.array([0.5, np.nan, -1.5, np.inf, -np.inf, 2.0, -0.0, 0.0, 5e-324, neg_nan, 0.5])
    assert np.signbit(s[9]) and not np.signbit(s[1])
    want = [3, 5, 0, 10, 8, 6, 7, 2, 4, 1, 9]
    assert np.argsort(-s, kind="mergesort").tolist() == want
    assert expected_order(s).tolist() == want
    assert np.lexsort((np.arange(len(s)), -s)).tolist() == want
    # with categories: NaN last inside its category only
    cat = np.array([1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1])
    assert expected_order(s, cat).tolist() == [3, 5, 7, 1, 9, 0, 10, 8, 6, 2, 4]


@pytest.mark.parametrize("kind", KINDS)
def test_populations_hold_what_they_name(kind):
    n = 4000
    s = score_population(kind, n, np.random.default_rng(3))
    again = score_population(kind, n, np.random.default_rng(3))
    assert scorepop.same_doubles(s, again)
    if kind == "logits":
        assert (s < 0).sum() > n // 3 and (s > 1).sum() > n // 3
        assert len(np.unique(s[s < 0])) < (s < 0).sum() and len(np.unique(s[s > 0])) < (s > 0).sum()
    if kind == "wide":
        tiny = np.abs(s) < 2.2250738585072014e-308
        assert tiny.sum() > 10 and (s[tiny] != 0).all()            # subnormals
        assert np.abs(s).max() > 1e300 and (s < 0).any() and np.isfinite(s).all()
    if kind == "specials":
        for v in scorepop.SPECIALS:
            share = (bits(s) == bits(np.array([v]))[0]).mean()
            assert 0.03 < share < 0.12, v
    if kind == "nan":
        for b in NAN_BITS:
            assert (bits(s) == b).sum() > 20
        assert 0.03 < np.isnan(s).mean() < 0.08
        cat_off = np.array([0, 100, 101, 101, 1500, 4000])
        s = score_population(kind, n, np.random.default_rng(3), cat_off, nan_cats=(4, 0))
        assert np.isnan(s[1500:]).all() and np.isnan(s[:100]).sum() == 99
    # a small column holds every special value as well
    small = score_population(kind, 24, np.random.default_rng(5))
    if kind == "nan":
        assert set(NAN_BITS.tolist()) <= set(bits(small).tolist())
    if kind == "specials":
        assert set(bits(scorepop.SPECIALS).tolist()) <= set(bits(small).tolist())


@pytest.mark.parametrize("kind", KINDS)
def test_host_sorter_on_any_double(kind):
    """flatten.sort_key_score (the native host sorter from 50000 elements on,
    numpy below) == the expectation."""
    for n, n_cat in ((60000, 40), (3000, 7)):
        rng = np.random.default_rng(n + KINDS.index(kind))
        cat = np.sort(rng.integers(0, n_cat, n))
        cat_off = np.searchsorted(cat, np.arange(n_cat + 1))
        s = score_population(kind, n, rng, cat_off)
        assert np.array_equal(fl.sort_key_score(cat, s), expected_order(s, cat))


@pytest.mark.parametrize("kind", KINDS)
def test_c_oracle_orders_any_double_like_numpy(kind):
    """orc_accumulate's own sort (the yardstick of the GPU tests) on a synth
    set whose scores are the population."""
    gt, dt, max_dets = scorepop.synth_with_scores("cells", kind)
    f = fl.flatten_lvis(gt, dt, max_dets)
    out = orclib.run_flat(f, detail=False)
    assert np.array_equal(out["order"], expected_order(f.dt_score, f.dt_cat))
    dt.track_id, _ = fl.make_track_ids_unique(dt)
    f = fl.flatten_tao(gt, dt, max_dets)
    out = orclib.run_flat(f, detail=False)
    assert np.array_equal(out["order"], expected_order(f.dt_score, f.dt_cat))


def _pyoracle_cut(dt, max_dets):
    anns = [{"image_id": int(i), "score": float(s), "_pos": k}
            for k, (i, s) in enumerate(zip(dt.image_id.tolist(), dt.score.tolist()))]
    return [a["_pos"] for a in pyoracle.limit_dets_per_image(anns, max_dets)]


def test_the_cut_inside_a_run_of_equal_scores_keeps_the_first_in_file_order():
    """Python's sorted(reverse=True) is stable: of equal negatives, equal +inf
    and -0.0 / 0.0 the first ones in the file stay (scorepop.TIE_IMAGES)."""
    gt, dt, max_dets, kept = scorepop.tie_cut_set()
    keep = fl.limit_dets_per_image(dt, max_dets)
    assert sorted(keep.tolist()) == kept
    assert keep.tolist() == _pyoracle_cut(dt, max_dets)
    f = fl.flatten_lvis(gt, dt, max_dets)
    assert sorted(map(tuple, np.asarray(f.dt_box).tolist())) == sorted(map(tuple, dt.bbox[kept].tolist()))
    # every track of the set has one box, one of them a NaN score: one score
    # each (the reference's set of a single NaN has one element), no average
    f = fl.flatten_tao(gt, dt, max_dets)
    assert not f.required_average and np.isnan(list(f.track_scores.values())).sum() == 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", list(scorepop.SYNTH_SETS))
def test_flatten_cut_equals_pyoracle_cut(which, kind):
    """limit_dets_per_image of flatten.py against oracle/pyoracle.py (the
    reference's sorted(..., reverse=True)[:max_dets]) on the sets the GPU
    tests build their tables from.  NaN scores lie only in images of at most
    max_dets detections (scorepop.synth_with_scores says why)."""
    gt, dt, max_dets = scorepop.synth_with_scores(which, kind)
    cnt = np.unique(dt.image_id, return_counts=True)[1]
    assert (cnt <= max_dets).any() and ((cnt > max_dets).any() or which == "cells")
    assert fl.limit_dets_per_image(dt, max_dets).tolist() == _pyoracle_cut(dt, max_dets)


@pytest.fixture(scope="module")
def long_set():
    return scorepop.long_track_set()


def test_long_tracks_mean_is_numpys_pairwise_sum_in_list_order(long_set):
    """flatten_tao's track score == np.mean of the track's scores in the order
    of the reference's list (images in first-seen order, file order inside),
    bit for bit, for tracks of 1 to 2051 boxes; a track of one score keeps it
    (the first box's: -0.0 and 0.0 are one element of the reference's set);
    +inf and -inf give NaN."""
    gt, dt = long_set
    f = fl.flatten_tao(gt, dt)
    order = np.asarray(_pyoracle_cut(dt, 300))
    assert len(order) == len(dt)
    trk, sc = dt.track_id[order], dt.score[order]
    n_box = np.bincount(dt.track_id)[1:]
    assert n_box.tolist() == scorepop.LONG_COUNTS + [300, 200, 200]
    differ = False
    for t in range(1, len(n_box) + 1):
        mine = sc[trk == t]
        if len(set(mine.tolist())) > 1:
            differ = True
            want = np.mean(mine)
        else:
            want = mine[0]
        assert scorepop.same_values([f.track_scores[t]], [want]), (t, len(mine))
    assert differ and f.required_average
    assert f.track_scores[len(scorepop.LONG_COUNTS) + 1] == -3.75
    assert f.track_scores[len(scorepop.LONG_COUNTS) + 2] == 0.0
    assert np.isnan(f.track_scores[len(scorepop.LONG_COUNTS) + 3])
    # another summation order does change these means: the test can fail
    t = scorepop.LONG_COUNTS.index(2051) + 1
    mine = sc[trk == t]
    assert float(np.sum(mine[::-1]) / len(mine)) != f.track_scores[t] or \
        float(sum(mine.tolist()) / len(mine)) != f.track_scores[t]


def test_tracks_of_one_score_need_no_average(long_set):
    """required_average follows the reference's rule (more than one element in
    the set of a track's scores): -0.0 and 0.0 are one element."""
    gt, dt = long_set
    n = len(scorepop.LONG_COUNTS)
    only = dt.take(np.flatnonzero((dt.track_id == n + 1) | (dt.track_id == n + 2)))
    f = fl.flatten_tao(gt, only)
    assert not f.required_average
    # (the element the set keeps is the first one put in: the track's first
    # box in list order, with its sign)
    order = np.asarray(_pyoracle_cut(only, 300))
    first = only.score[order][only.track_id[order] == n + 2][0]
    assert scorepop.same_doubles([f.track_scores[n + 1], f.track_scores[n + 2]], [-3.75, first])
