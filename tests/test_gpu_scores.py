"""-m gpu: eval["scores"] -- the score at which recall first reaches each recall
threshold (pycocotools' ss[ri] = dtScoresSorted[pi], read at the reference's
rec_thrs_insert_idx, lvis_amodal/eval.py:406-417 == tao_amodal/eval.py:562-573)
-- against the numpy restatement of tests/score_ref.py: the class API on the
reference's recorded runs, taoamd_score_at_recall on synthetic rows over every
boundary of its blocking, and the error paths.  A value is a copy of an input
score: every comparison is exact."""
import sys

import numpy as np
import pytest

import score_ref
import wsguard
from goldenio import GOLDEN as GOLDEN_DIR, load_eval, load_inputs, load_lvis_nocats, \
    load_modes, path
from tao_amodal_amd import _lib

sys.path.insert(0, GOLDEN_DIR)
from constants_cases import cases, edit  # noqa: E402

pytestmark = pytest.mark.gpu

N_THR, N_REC = _lib.N_THR, _lib.N_REC
REC_THRS = np.linspace(0.0, 1.0, 101)
GOLDEN = ["f1", "f2", "f4", "f9"]


def _lvis(name, iou_type="bbox", pred="pred.json"):
    from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
    return LVISEval(path(name, "gt.json"), path(name, pred), iou_type)


def _tao(name, **kw):
    from tao_amodal_amd import flatten
    from tao_amodal_amd.columns import DTColumns
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval, TaoResults
    dt = DTColumns.from_json(path(name, "pred.json"))
    dt.track_id, _ = flatten.make_track_ids_unique(dt)
    gt = Tao(path(name, "gt.json"))
    return TaoEval(gt, TaoResults(gt, dt), **kw)


def _scores_of(ev, want_p, problem=None):
    """evaluate + accumulate + score_at_recall; the invariants every case
    shares.  `problem` None: the restatement's inputs are the evaluator's own
    dt_pointers and its input scores, pinned to the golden precision by the
    envelope read at the restatement's insert index."""
    ev.evaluate()
    with pytest.raises(RuntimeError, match=r"Please run accumulate\(\) first\."):
        ev.score_at_recall()
    ev.accumulate()
    assert "scores" not in ev.eval
    p0, r0 = ev.eval["precision"].copy(), ev.eval["recall"].copy()
    assert np.array_equal(p0, want_p)
    got = ev.score_at_recall()
    assert ev.eval["scores"] is got and ev.score_at_recall() is got
    assert got.shape == p0.shape and got.dtype == np.float64
    assert np.array_equal(ev.eval["precision"], p0) and np.array_equal(ev.eval["recall"], r0)
    assert np.array_equal(got == -1, want_p == -1)
    flat4 = p0.shape[:3] + (int(np.prod(p0.shape[3:])),)
    rec = np.asarray(ev.params.rec_thrs, dtype=np.float64)
    if problem is None:
        f = ev._run.flat
        by_id = dict(zip(np.asarray(f.dt_id).tolist(), np.asarray(f.dt_score).tolist()))
        n_time = p0.shape[4] if p0.ndim == 5 else None
        problem = score_ref.pointers_problem(ev, by_id, flat4[3], n_time)
        assert np.array_equal(score_ref.table(problem, flat4, rec, precision=True),
                              want_p.reshape(flat4))
    want = score_ref.table(problem, flat4, rec)
    assert np.array_equal(got.reshape(flat4), want)
    return got


@pytest.mark.parametrize("name", GOLDEN)
def test_lvis_eval_scores_on_the_reference_goldens(name):
    ev = _lvis(name)
    got = _scores_of(ev, load_eval(name)["lvis"][0], score_ref.golden_problem(name, "lvis"))
    pts = ev.operating_points(0.5, 0.5)
    assert pts == {c: got[0, 50, k, 0] for k, c in enumerate(ev.params.cat_ids)
                   if got[0, 50, k, 0] != -1} and pts


@pytest.mark.parametrize("name", GOLDEN)
def test_tao_eval_scores_on_the_reference_goldens(name):
    ev = _tao(name)
    got = _scores_of(ev, load_eval(name)["tao"][0], score_ref.golden_problem(name, "tao"))
    assert got.ndim == 5 and got.shape[3:] == (5, 4)
    pts = ev.operating_points(0.75, 0.1, rng=("all", "all"))
    assert pts == {c: got[5, 10, k, 0, 0] for k, c in enumerate(ev.params.cat_ids)
                   if got[5, 10, k, 0, 0] != -1}


def test_the_golden_problem_is_also_the_evaluators_own():
    """The two sources of the restatement's inputs agree where both exist."""
    ev = _lvis("f1")
    ev.evaluate()
    ev.accumulate()
    f = ev._run.flat
    by_id = dict(zip(np.asarray(f.dt_id).tolist(), np.asarray(f.dt_score).tolist()))
    own = score_ref.pointers_problem(ev, by_id, 6)
    want = score_ref.golden_problem("f1", "lvis")
    assert own.keys() == want.keys()
    for key, (tps, fps, sc, ng) in want.items():
        assert np.array_equal(own[key][0], tps) and np.array_equal(own[key][2], sc)
        assert own[key][3] == ng


@pytest.mark.parametrize("name", ["f1", "f4"])
def test_scores_without_categories(name):
    """params.use_cats = 0 on both levels: one pooled category."""
    ev = _lvis(name)
    ev.params.use_cats = 0
    got = _scores_of(ev, load_lvis_nocats(name)[2])
    assert got.shape[2] == 1 and set(ev.operating_points(0.5, 0.3)) <= {-1}
    te = _tao(name)
    te.params.use_cats = 0
    got = _scores_of(te, load_modes(name)["nocats"][1])
    assert got.shape[2] == 1


def test_scores_of_mask_ious():
    """iou_type="segm" (f6): the rows are shared with the box path."""
    z = np.load(path("f6", "lvis_segm.npz"))
    _scores_of(_lvis("f6", "segm", "pred_rle.json"), z["pred_rle_precision"])


@pytest.mark.parametrize("case", ["few", "unsorted_rec"])
def test_scores_under_edited_constants_of_one_block(case):
    """Fewer thresholds than the kernels' blocks in the caller's (unsorted)
    order; recall thresholds out of order: what follows the first unreached one
    stays 0, like the reference's precision."""
    z = np.load(path("f1", "constants.npz"))
    ev = _lvis("f1")
    edit(ev.params, cases()[case], "lvis")
    got = _scores_of(ev, z[case + "_lvis_precision"])
    assert got.shape[:2] == (len(ev.params.iou_thrs), len(ev.params.rec_thrs))
    te = _tao("f1")
    edit(te.params, cases()[case], "tao")
    _scores_of(te, z[case + "_tao_precision"])


def test_several_blocks_of_constants_are_refused():
    ev = _lvis("f1")
    edit(ev.params, cases()["many"], "lvis")
    ev.evaluate()
    ev.accumulate()
    with pytest.raises(NotImplementedError, match=r"eval\['scores'\] is kept for up to 10 IoU"):
        ev.score_at_recall()
    assert "scores" not in ev.eval
    with pytest.raises(RuntimeError, match=r"score_at_recall\(\) first"):
        ev.operating_points(0.5, 0.5)


# ---------------------------------------------------------------------------
# taoamd_score_at_recall on synthetic rows
# ---------------------------------------------------------------------------
# (rows, TP density) of the categories: every boundary of the 64-row blocks and
# the 256-row chunks at 0, ~5 % and 100 %; 5000 rows (20 chunks) sparse, 2600
# (11 chunks) dense, and 9000 rows (36 chunks: a quarter of them is more than
# the eight chunks the prefix kernel takes per step) sparse
CATS = [(0, 0.05), (1, 1.0), (63, 0.05), (64, 1.0), (65, 0.0), (255, 0.05), (256, 1.0),
        (257, 0.05), (511, 1.0), (512, 0.05), (513, 0.0), (1025, 1.0), (5000, 0.05),
        (0, 1.0), (300, 0.05), (9000, 0.05), (2600, 1.0)]
SIZES = [n for n, _ in CATS]
LONG = [k for k, (n, _) in enumerate(CATS) if n >= 5000]


@pytest.fixture(scope="module")
def synthetic():
    """{n_rng: (cat_off, matched, ignored, scores, num_gt, want)}: categories on
    every boundary of the 64-row blocks and the 256-row chunks, of 11, 20 and
    36 chunks; TP density 0, ~5 % and 100 %; num_gt 0, below, at and above what the
    category reaches; first rows that are no TP; scores in runs of equal values
    that straddle the chunk boundaries, the tail of every category negative."""
    out = {}
    for n_rng in (6, 20):
        rng = np.random.default_rng(100 + n_rng)
        n_combo = n_rng * N_THR
        nw = (n_combo + 63) // 64
        cat_off = np.zeros(len(SIZES) + 1, np.int32)
        np.cumsum(SIZES, out=cat_off[1:])
        n, K = int(cat_off[-1]), len(SIZES)
        m_bits = np.zeros((n, nw * 64), bool)
        i_bits = rng.random((n, nw * 64)) < 0.1
        scores = np.zeros(n)
        num_gt = np.zeros((K, n_rng), np.int32)
        for k, (lo, hi) in enumerate(zip(cat_off[:-1], cat_off[1:])):
            d = CATS[k][1]
            m_bits[lo:hi] = rng.random((hi - lo, nw * 64)) < d if d < 1 else True
            if hi > lo and k % 2:
                m_bits[lo] = False                       # the first row is no TP
            # runs of ~100 equal scores, descending, the last fifth below zero
            s = np.sort(np.floor(rng.random(hi - lo) * ((hi - lo) // 100 + 2)))[::-1]
            scores[lo:hi] = s / 8 - 0.2 * (s.max() / 8 if hi > lo else 0)
            tp = (m_bits[lo:hi] & ~i_bits[lo:hi])[:, :n_combo].sum(0).reshape(n_rng, N_THR)
            for r in range(n_rng):
                top = int(tp[r].max())
                num_gt[k, r] = [0, max(top // 2, 1), max(top, 1), 2 * top + 3,
                                int(rng.integers(1, 40))][(k + r) % 5]
        assert (scores < 0).any()
        for k in LONG:
            # equal scores across (nearly all) chunk boundaries; TPs in (nearly) every chunk of every combo
            lo, hi = int(cat_off[k]), int(cat_off[k + 1])
            across = np.diff(scores[lo:hi])[255::256] == 0
            assert across.sum() >= 15 and across.mean() > 0.8
            per_chunk = np.add.reduceat((m_bits[lo:hi] & ~i_bits[lo:hi])[:, :n_combo],
                                        np.arange(0, hi - lo, 256))
            assert (per_chunk > 0).mean() > 0.99
        matched = np.packbits(m_bits, axis=1, bitorder="little").view(np.uint64)
        ignored = np.packbits(i_bits, axis=1, bitorder="little").view(np.uint64)
        tps = m_bits & ~i_bits
        want = -np.ones((N_THR, N_REC, K, n_rng))
        for k, (lo, hi) in enumerate(zip(cat_off[:-1], cat_off[1:])):
            for r in range(n_rng):
                if num_gt[k, r] > 0:
                    want[:, :, k, r] = score_ref.score_at_recall(
                        tps[lo:hi, r * N_THR:(r + 1) * N_THR].T, scores[lo:hi],
                        int(num_gt[k, r]), REC_THRS)
        live = want[want != -1]
        assert (live == 0).any() and (live < 0).any() and (live > 0).any()
        for k in LONG:
            # thresholds are crossed all along the long categories: rows of the
            # last chunks are selected (their scores are the negative ones)
            assert len(np.unique(want[:, :, k])) > 20 and (want[:, :, k] < 0).any()
        for a in (cat_off, matched, ignored, scores, num_gt, want):
            a.setflags(write=False)
        out[n_rng] = (cat_off, matched, ignored, scores, num_gt, want)
    return out


def _device_scores(cat_off, matched, ignored, scores, num_gt, order, layout,
                   score_order=None):
    """taoamd_score_at_recall on the rows (and scores) stored at order[p]; with
    `score_order` the scores lie at score_order[p] instead."""
    import torch
    lib = _lib.load()
    dev = "cuda:0"
    K, n_rng = num_gt.shape
    n, nw = matched.shape
    m_at, i_at, s_at = matched, ignored, scores
    if order is not None:
        m_at, i_at, s_at = np.empty_like(matched), np.empty_like(ignored), np.empty_like(scores)
        m_at[order], i_at[order], s_at[order] = matched, ignored, scores
    if score_order is not None:
        s_at = np.empty_like(scores)
        s_at[score_order] = scores
    d_sorder = None if score_order is None else torch.from_numpy(score_order).to(dev)
    d_off = torch.from_numpy(np.array(cat_off)).to(dev)
    d_ng = torch.from_numpy(np.array(num_gt)).to(dev)
    d_sc = torch.from_numpy(np.array(s_at)).to(dev)
    d_order = None if order is None else torch.from_numpy(order).to(dev)
    if layout == "paired":
        rows = torch.empty((n, nw, 2), dtype=torch.int64, device=dev)
        rows[:, :, 0] = torch.from_numpy(np.array(m_at).view(np.int64)).to(dev)
        rows[:, :, 1] = torch.from_numpy(np.array(i_at).view(np.int64)).to(dev)
        d_m, d_i = rows[..., 0], rows[..., 1]
    else:
        d_m = torch.from_numpy(np.array(m_at).view(np.int64)).to(dev)
        d_i = torch.from_numpy(np.array(i_at).view(np.int64)).to(dev)
    ws = wsguard.Guarded(lib.taoamd_score_at_recall_workspace(n, K, n_rng), dev)
    out = torch.full((N_THR, N_REC, K, n_rng), 7.0, dtype=torch.float64, device=dev)
    _lib.check(lib.taoamd_score_at_recall(
        n, K, n_rng, d_off.data_ptr(), None if d_order is None else d_order.data_ptr(),
        d_m.data_ptr(), d_i.data_ptr(), d_sc.data_ptr(),
        None if d_sorder is None else d_sorder.data_ptr(), d_ng.data_ptr(), out.data_ptr(),
        ws.data_ptr(), ws.nbytes, torch.cuda.current_stream().cuda_stream),
        "taoamd_score_at_recall")
    ws.check()
    return out.cpu().numpy()


@pytest.mark.parametrize("layout", ["paired", "split"])
@pytest.mark.parametrize("how", ["sorted", "cell_order", "shuffled"])
@pytest.mark.parametrize("n_rng", [6, 20])
def test_abi_on_every_boundary_of_the_blocking(synthetic, n_rng, how, layout):
    cat_off, matched, ignored, scores, num_gt, want = synthetic[n_rng]
    rng = np.random.default_rng(7)
    n = int(cat_off[-1])
    order = None
    if how == "shuffled":
        order = rng.permutation(n).astype(np.int32)
    elif how == "cell_order":            # a category's rows stay one piece
        order = np.arange(n, dtype=np.int32)
        for a, b in zip(cat_off[:-1], cat_off[1:]):
            order[a:b] = a + rng.permutation(int(b - a))
    got = _device_scores(cat_off, matched, ignored, scores, num_gt, order, layout)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("how", ["sorted", "cell_order"])
def test_abi_with_scores_in_a_numbering_of_their_own(synthetic, how):
    """score_order: rows in sorted places (or at order[p]) beside scores that
    lie where the detections are -- what the engine passes."""
    cat_off, matched, ignored, scores, num_gt, want = synthetic[6]
    rng = np.random.default_rng(11)
    n = int(cat_off[-1])
    order = rng.permutation(n).astype(np.int32) if how == "cell_order" else None
    got = _device_scores(cat_off, matched, ignored, scores, num_gt, order, "paired",
                         score_order=rng.permutation(n).astype(np.int32))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_abi_with_the_workspace_base_moved_by_8_bytes(synthetic, monkeypatch):
    monkeypatch.setattr(wsguard, "SHIFT", 8)
    test_abi_on_every_boundary_of_the_blocking(synthetic, 20, "cell_order", "paired")


def test_abi_under_the_callers_recall_thresholds(synthetic):
    """The calling thread's thresholds (taoamd_set_thresholds), several of them
    equal (a short block padded with its last value) and several at recall 0."""
    cat_off, matched, ignored, scores, num_gt, _ = synthetic[6]
    rec = np.concatenate([np.zeros(3), np.linspace(0.01, 0.97, 90), np.full(8, 0.97)])
    _lib.set_constants(rec_thrs=rec)
    try:
        got = _device_scores(cat_off, matched, ignored, scores, num_gt, None, "paired")
    finally:
        _lib.set_constants()
    m = np.unpackbits(np.array(matched).view(np.uint8), axis=1, bitorder="little").astype(bool)
    i = np.unpackbits(np.array(ignored).view(np.uint8), axis=1, bitorder="little").astype(bool)
    tps = m & ~i
    for k, (lo, hi) in enumerate(zip(cat_off[:-1], cat_off[1:])):
        for r in range(6):
            want = -np.ones((N_THR, N_REC)) if num_gt[k, r] == 0 else \
                score_ref.score_at_recall(tps[lo:hi, r * N_THR:(r + 1) * N_THR].T,
                                          scores[lo:hi], int(num_gt[k, r]), rec)
            assert np.array_equal(got[:, :, k, r], want), (k, r)


def test_engine_stage_on_rows_in_cell_order():
    """engine.stage_scores behind both forms of a pass: rows scattered to their
    sorted places, and rows left in cell order with the sweep gathering them."""
    import torch
    from tao_amodal_amd import engine, flatten as fl
    from tao_amodal_amd.columns import DTColumns, GTColumns
    gtj, predj = load_inputs("f4")
    f = fl.flatten_lvis(GTColumns.from_json(gtj), DTColumns.from_json(predj))
    dp = engine.DeviceProblem(f, "cuda:0")
    ws = engine.Workspace(dp, keep_order=True)
    tables = []
    for scatter in (True, False):
        engine.stage_ranges(dp, ws)
        engine.stage_sort(dp, ws)
        engine.stage_match(dp, ws, scatter=scatter)
        (engine.stage_accumulate if scatter else engine.stage_accumulate_by_order)(dp, ws)
        engine.stage_scores(dp, ws)
        torch.cuda.synchronize()
        assert ws.cell_order == (not scatter)
        tables.append(ws.scores.cpu().numpy())
    want = score_ref.table(score_ref.golden_problem("f4", "lvis"), tables[0].shape, REC_THRS)
    assert np.array_equal(tables[0], want) and np.array_equal(tables[1], want)
