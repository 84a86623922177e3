"""-m gpu: every device stage that looks at a score, on scores that are any
double (tests/scorepop.py: logits, subnormals to near overflow, +-inf, +-0.0,
+-DBL_MAX, NaN in three bit patterns) and on tracks of up to 2051 boxes.
The expected order is numpy's, np.lexsort((arange, -score, cat)): every NaN
last in input order (pinned on the host in test_score_values_host.py).  All
comparisons are exact: == on integers, bit patterns on doubles.

The exchange kernels run on the same populations in test_gpu_parity.py, the
reference's recorded run on such scores (fixture f10) in the golden tests of
test_gpu_parity.py, test_gpu_flatten.py and test_gpu_cli.py."""
import numpy as np
import pytest

import score_ref
import scorepop
import wsguard
from goldenio import SCORE_FIXTURES, load_eval
from scorepop import KINDS, expected_order, score_population
from tao_amodal_amd import _lib

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# the three sorts through the ABI
# ---------------------------------------------------------------------------
def _offsets(sizes):
    cat_off = np.zeros(len(sizes) + 1, np.int32)
    np.cumsum(sizes, out=cat_off[1:])
    tiles = (np.diff(cat_off) + _lib.SEGMENT_TILE - 1) // _lib.SEGMENT_TILE
    tile_off = np.zeros(len(sizes) + 1, np.int32)
    np.cumsum(tiles, out=tile_off[1:])
    return cat_off, tile_off


def _first_difference(got, want):
    d = np.flatnonzero(got != want)
    return "equal" if len(d) == 0 else "first differing index %d: got %d, want %d (%d differ)" % (
        d[0], got[d[0]], want[d[0]], len(d))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,n_cat", [(60000, 40), (30000, 1)])
def test_radix_and_segment_sort_on_any_double(n, n_cat, kind):
    """taoamd_sort_by_cat_score and taoamd_sort_segments: keys on both sides
    of the sign bit, ties on both sides of zero, subnormals that must survive
    the key's s + 0.0, NaN of either sign last."""
    import torch
    lib = _lib.load()
    rng = np.random.default_rng(n + n_cat + KINDS.index(kind))
    cat = np.sort(rng.integers(0, n_cat, n)).astype(np.int32)
    cat_off, tile_off = _offsets(np.bincount(cat, minlength=n_cat))
    score = score_population(kind, n, rng, cat_off)
    want = expected_order(score, cat)
    d_cat, d_score = torch.from_numpy(cat).cuda(), torch.from_numpy(score).cuda()
    order = torch.empty(n, dtype=torch.int32, device="cuda")
    dst = torch.empty(n, dtype=torch.int32, device="cuda")
    ws = wsguard.Guarded(lib.taoamd_sort_workspace(n))
    _lib.check(lib.taoamd_sort_by_cat_score(n, d_cat.data_ptr(), d_score.data_ptr(),
                                            order.data_ptr(), dst.data_ptr(),
                                            ws.data_ptr(), ws.nbytes, None), "radix")
    ws.check()
    got = order.cpu().numpy()
    assert np.array_equal(got, want), _first_difference(got, want)
    assert np.array_equal(dst.cpu().numpy()[want], np.arange(n))
    order.zero_(); dst.zero_()
    d_co, d_to = torch.from_numpy(cat_off).cuda(), torch.from_numpy(tile_off).cuda()
    ws = wsguard.Guarded(lib.taoamd_sort_segments_workspace(n))
    _lib.check(lib.taoamd_sort_segments(
        n, n_cat, d_co.data_ptr(), d_to.data_ptr(), int(tile_off[-1]),
        int(np.diff(cat_off).max()), d_cat.data_ptr(), d_score.data_ptr(),
        order.data_ptr(), dst.data_ptr(), ws.data_ptr(), ws.nbytes, None), "segments")
    ws.check()
    got = order.cpu().numpy()
    assert np.array_equal(got, want), _first_difference(got, want)
    assert np.array_equal(dst.cpu().numpy()[want], np.arange(n))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("limit", [0, 40])
def test_sample_sort_on_any_double(limit, kind):
    """taoamd_sort_sampled on the categories of
    test_sample_sort_every_kind_of_category (empty, one wavefront, around the
    direct limit, bucket split, one chunk, chunk + 1, several chunks): the
    key range crosses the sign bit, so the key parts are shifted furthest and
    tie, splitters lie on either side of zero, and -- limit 40 -- the
    counting path ranks these keys too.  "nan": the category of 1300 is all
    NaN, that of 2817 all NaN but one element."""
    import torch
    from test_gpu_parity import _sampled_sort
    lib = _lib.load()
    rng = np.random.default_rng(31 + KINDS.index(kind))
    chunk = 16 * _lib.SEGMENT_TILE
    sizes = [0, 1, 63, 64, 65, 129, 500, 1024, 1025, 1300, 0, 2816, 2817, 9000,
             chunk, chunk + 1, 3 * chunk + 77, 20000, 7]
    if limit:
        sizes = [0, 1, 65, 500, 1025, 1300, 2817, 5000, 7]
    n, n_cat = int(np.sum(sizes)), len(sizes)
    cat = np.repeat(np.arange(n_cat), sizes)
    cat_off, tile_off = _offsets(sizes)
    score = score_population(kind, n, rng, cat_off,
                             nan_cats=(sizes.index(1300), sizes.index(2817)))
    want = expected_order(score, cat)
    d_score = torch.from_numpy(score).cuda()
    try:
        lib.taoamd_sort_sampled_cap_limit(limit)
        order, dst = _sampled_sort(cat_off, tile_off, d_score, repeat=2)
    finally:
        lib.taoamd_sort_sampled_cap_limit(0)
    assert np.array_equal(order, want), _first_difference(order, want)
    assert np.array_equal(dst[want], np.arange(n))


# ---------------------------------------------------------------------------
# the device table build
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", list(scorepop.SYNTH_SETS))
def test_lvis_device_tables_on_any_double(which, kind):
    """flatten_lvis_device against flatten.py, field by field, then the
    evaluation against the oracle: the order inside the cells and the cut at
    max_dets use the sorts' key.  NaN scores go only into images of at most
    max_dets detections: the order Python's sorted() gives a list that holds
    NaNs depends on the input order and is no rule worth restating."""
    from test_gpu_flatten import _lvis_both
    gt, dt, max_dets = scorepop.synth_with_scores(which, kind)
    _lvis_both(gt, dt, max_dets)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", list(scorepop.SYNTH_SETS))
def test_tao_device_tables_on_any_double(which, kind):
    """flatten_tao_device against flatten.py (tables, track scores,
    required_average), then the evaluation against the oracle.  NaN scores:
    see test_lvis_device_tables_on_any_double."""
    from test_gpu_flatten import _tao_both
    gt, dt, max_dets = scorepop.synth_with_scores(which, kind)
    _tao_both(gt, dt, max_dets)


def test_device_cut_inside_a_run_of_equal_scores_keeps_the_first_in_file_order():
    """Equal negatives, equal +inf, -0.0 / 0.0 at the cut (scorepop.TIE_IMAGES):
    the kept boxes are the first ones in file order, on both levels."""
    from test_gpu_flatten import _lvis_both, _tao_both
    from tao_amodal_amd import flatten_dev
    gt, dt, max_dets, kept = scorepop.tie_cut_set()
    want = sorted(map(tuple, dt.bbox[kept].tolist()))
    got = flatten_dev.flatten_lvis_device(gt, dt, "cuda:0", max_dets)
    assert sorted(map(tuple, np.asarray(got["dt_box"]).tolist())) == want
    _lvis_both(gt, dt, max_dets)
    got = flatten_dev.flatten_tao_device(gt, dt, "cuda:0", max_dets)
    assert sorted(map(tuple, np.asarray(got["dt_frame_box"]).tolist())) == want
    _tao_both(gt, dt, max_dets)


def test_long_tracks_mean_on_the_device():
    """Tracks of 1 to 2051 kept boxes (scorepop.long_track_set): the device's
    restatement of numpy's pairwise summation, its recursion above 128 boxes,
    the 8-aligned split and the tail, on scores whose mean changes with the
    order of the additions; the one-score shortcut with -0.0 and 0.0 mixed;
    a mean that is NaN.  track_scores, dt_score and required_average equal
    flatten.py's (pinned to np.mean on the host), the evaluation the oracle's."""
    from test_gpu_flatten import _tao_both
    gt, dt = scorepop.long_track_set()
    _tao_both(gt, dt)


# ---------------------------------------------------------------------------
# eval["scores"]
# ---------------------------------------------------------------------------
def _scores_with_markers(ev, want_p, problem):
    """score_at_recall() of an evaluator against the restatement, bit for bit.
    Returns (table, reached): reached[T, R, K, ...] says whether the final
    recall of the column reaches the recall threshold -- the only thing that
    tells a real score of 0.0 from the 0 of "never reached"; a real score of
    -1.0 differs from the -1 of "no ground truth" by the precision table's -1
    alone.  The table itself cannot tell them apart (inherited from
    pycocotools); nothing here gives them another encoding."""
    ev.evaluate()
    ev.accumulate()
    p0, r0 = ev.eval["precision"], ev.eval["recall"]
    assert np.array_equal(p0, want_p)
    got = ev.score_at_recall()
    flat4 = p0.shape[:3] + (int(np.prod(p0.shape[3:])),)
    rec = np.asarray(ev.params.rec_thrs, dtype=np.float64)
    want = score_ref.table(problem, flat4, rec)
    assert scorepop.same_doubles(got.reshape(flat4), want)
    # every entry is a marker or a bit-exact copy of an input score
    inputs = set(scorepop.bits(ev._run.flat.dt_score).tolist())
    markers = set(scorepop.bits(np.array([0.0, -1.0])).tolist())
    assert set(scorepop.bits(got.reshape(-1)).tolist()) <= inputs | markers
    # no ground truth -> -1 (the converse does not hold: a score may be -1.0)
    assert (got[p0 == -1] == -1).all()
    reached = r0[:, None] >= rec.reshape((1, -1) + (1,) * (p0.ndim - 2))
    return got, reached & (p0 != -1)


@pytest.mark.parametrize("name", SCORE_FIXTURES)
@pytest.mark.parametrize("side", ["lvis", "tao"])
def test_eval_scores_on_the_score_fixture(name, side):
    """f10: category 2's best detection scores exactly 0.0, category 3's -1.0.
    Both kinds of 0 and both kinds of -1 occur in the table; the recall and
    precision tables at those entries say which is which."""
    from test_gpu_scores import _lvis, _tao
    ev = _lvis(name) if side == "lvis" else _tao(name)
    got, reached = _scores_with_markers(ev, load_eval(name)[side][0],
                                        score_ref.golden_problem(name, side))
    zero, minus = got == 0, got == -1
    assert (zero & reached).any()          # a real score of 0.0 (or -0.0)
    assert (zero & ~reached & (ev.eval["precision"] != -1)).any()     # never reached
    assert (minus & reached).any()         # a real score of -1.0
    assert (minus & (ev.eval["precision"] == -1)).any()               # no ground truth
    # reached entries that are neither: other input scores, NaN and -inf among them
    rest = got[reached & ~zero & ~minus]
    assert np.isinf(rest).any() and (rest < 0).any()


from test_gpu_scores import synthetic  # noqa: E402,F401  (the module's fixture)


@pytest.mark.parametrize("kind", ["specials", "nan"])
def test_abi_on_the_blocking_boundaries_with_any_double(synthetic, kind):  # noqa: F811
    """taoamd_score_at_recall on the rows of test_gpu_scores.py (every boundary
    of the 64-row blocks and the 256-row chunks, rows in cell order), the
    scores drawn from a pool of the population so that runs of equal values
    straddle the chunks: each entry a bit-exact copy of the input score."""
    from test_gpu_scores import N_REC, N_THR, REC_THRS, _device_scores
    cat_off, matched, ignored, _, num_gt, _ = synthetic[6]
    rng = np.random.default_rng(17 + KINDS.index(kind))
    n, K = int(cat_off[-1]), len(cat_off) - 1
    scores = np.zeros(n)
    for lo, hi in zip(cat_off[:-1], cat_off[1:]):
        pool = score_population(kind, 30, rng)
        run = pool[rng.integers(0, len(pool), hi - lo)]
        scores[lo:hi] = run[expected_order(run)]
    m = np.unpackbits(np.array(matched).view(np.uint8), axis=1, bitorder="little").astype(bool)
    i = np.unpackbits(np.array(ignored).view(np.uint8), axis=1, bitorder="little").astype(bool)
    tps = m & ~i
    want = -np.ones((N_THR, N_REC, K, 6))
    for k, (lo, hi) in enumerate(zip(cat_off[:-1], cat_off[1:])):
        for r in range(6):
            if num_gt[k, r] > 0:
                want[:, :, k, r] = score_ref.score_at_recall(
                    tps[lo:hi, r * N_THR:(r + 1) * N_THR].T, scores[lo:hi],
                    int(num_gt[k, r]), REC_THRS)
    live = want[:, :, num_gt > 0]
    # (the case holds what it is about: markers and real special values)
    assert (live == 0).any() and (live < 0).any()
    assert np.isnan(live).any() if kind == "nan" else np.isinf(live).any()
    order = np.arange(n, dtype=np.int32)
    for a, b in zip(cat_off[:-1], cat_off[1:]):
        order[a:b] = a + rng.permutation(int(b - a))
    got = _device_scores(cat_off, matched, ignored, scores, num_gt, order, "paired")
    assert scorepop.same_doubles(got, want)
