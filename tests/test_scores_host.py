"""eval["scores"] without a GPU: the numpy restatement of the rule
(tests/score_ref.py) read at the reference's own recorded results, the host
helper operating_points(), and the C ABI's new symbols."""
import os
import re

import numpy as np
import pytest

import score_ref
from goldenio import load_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC_THRS = np.linspace(0.0, 1.0, 101)
GOLDEN = ["f1", "f2", "f4", "f9"]


@pytest.mark.parametrize("side", ["lvis", "tao"])
@pytest.mark.parametrize("name", GOLDEN)
def test_the_insert_index_is_the_references(name, side):
    """The precision envelope read at the restatement's insert index is the
    golden precision bit for bit (the recorded dt_pointers, num_gt from the
    recorded gt_ignore): the index rule is the reference's.  The score is then
    dt_scores at that same index, and it is one of the category's scores, in
    non-increasing order along the recall axis while it is reached."""
    want_p = load_eval(name)[side][0]
    shape = want_p.shape[:3] + (int(np.prod(want_p.shape[3:])),)
    want_p = want_p.reshape(shape)
    problem = score_ref.golden_problem(name, side)
    assert problem
    assert np.array_equal(score_ref.table(problem, shape, REC_THRS, precision=True), want_p)
    scores = score_ref.table(problem, shape, REC_THRS)
    assert np.array_equal(scores == -1, want_p == -1)
    for (k, a), (tps, fps, sc, num_gt) in problem.items():
        got = scores[:, :, k, a]
        assert np.isin(got, np.concatenate([sc, [0.0]])).all()
        for t in range(len(tps)):
            reached = int(np.count_nonzero(
                score_ref.insert_index(tps[t], num_gt, REC_THRS) < len(sc)))
            assert (np.diff(got[t, :reached]) <= 0).all()
            assert (got[t, reached:] == 0).all()
            if reached:
                assert got[t, 0] == sc[0]          # recall 0: the first row


def test_restatement_on_a_hand_made_category():
    tps = np.array([[0, 1, 0, 1, 1], [0, 0, 0, 0, 0]], dtype=bool)
    sc = np.array([0.9, 0.8, 0.8, 0.5, -0.25])
    rec = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    got = score_ref.score_at_recall(tps, sc, 4, rec)
    # 4 GT: 1 TP reaches 0.25 at row 1, 2 at row 3, 3 at row 4, 4 never
    assert got.tolist() == [[0.9, 0.8, 0.5, -0.25, 0.0], [0.9, 0.0, 0.0, 0.0, 0.0]]
    # unsorted thresholds: everything after the first unreached one stays 0
    got = score_ref.score_at_recall(tps, sc, 4, np.array([0.5, 1.0, 0.25]))
    assert got[0].tolist() == [0.5, 0.0, 0.0]
    # no detections at all: the first read raises
    assert not score_ref.score_at_recall(np.zeros((2, 0), bool), np.zeros(0), 3, rec).any()


def _evaluator(cls, params_cls, scores, **params):
    ev = cls.__new__(cls)
    ev.params = params_cls("bbox")
    for k, v in params.items():
        setattr(ev.params, k, v)
    ev.eval = {"scores": scores}
    return ev


def test_operating_points_on_a_hand_made_eval():
    from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
    from tao_amodal_amd.evaluation.lvis_amodal.eval import Params as LP
    from tao_amodal_amd.evaluation.tao_amodal import TaoEval
    from tao_amodal_amd.evaluation.tao_amodal.eval import Params as TP
    rng = np.random.default_rng(5)
    s = rng.random((10, 101, 3, 6))
    s[:, :, 1, 0] = -1
    s[:, :, 2, 3] = -1
    ev = _evaluator(LVISEval, LP, s, cat_ids=[7, 3, 11])
    assert ev.operating_points(0.5, 0.9) == {7: s[0, 90, 0, 0], 11: s[0, 90, 2, 0]}
    iou75 = ev.params.iou_thrs[5]
    assert ev.operating_points(iou75, 1.0, rng="highly-visible") == \
        {7: s[5, 100, 0, 3], 3: s[5, 100, 1, 3]}
    with pytest.raises(ValueError):
        ev.operating_points(0.55000001, 0.9)
    with pytest.raises(ValueError):
        ev.operating_points(0.5, 0.905)
    with pytest.raises(ValueError):
        ev.operating_points(0.5, 0.9, rng="no such range")
    ev.params.use_cats = 0
    ev.eval["scores"] = s[:, :, :1]
    assert ev.operating_points(0.5, 0.0) == {-1: s[0, 0, 0, 0]}
    ev.eval = {"precision": s}
    with pytest.raises(RuntimeError):
        ev.operating_points(0.5, 0.9)
    t = rng.random((10, 101, 2, 5, 4))
    t[:, :, 0, 1, 2] = -1
    ev = _evaluator(TaoEval, TP, t, cat_ids=[4, 9])
    assert ev.operating_points(0.5, 0.5) == {4: t[0, 50, 0, 0, 0], 9: t[0, 50, 1, 0, 0]}
    assert ev.operating_points(0.5, 0.5, rng=("small", "medium")) == {9: t[0, 50, 1, 1, 2]}


def test_score_at_recall_wants_accumulate_first():
    from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
    from tao_amodal_amd.evaluation.tao_amodal import TaoEval
    for cls in (LVISEval, TaoEval):
        ev = cls.__new__(cls)
        ev.eval = {}
        with pytest.raises(RuntimeError, match=r"Please run accumulate\(\) first\."):
            ev.score_at_recall()


def test_a_multi_gpu_run_has_no_score_table():
    from tao_amodal_amd.evaluation._dist import DistRun
    with pytest.raises(NotImplementedError, match=r"eval\['scores'\] in a multi-GPU run"):
        DistRun.__new__(DistRun).score_table()


def test_abi_symbols_are_declared_exported_and_bound():
    from tao_amodal_amd import _lib
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in ("taoamd_score_at_recall_workspace", "taoamd_score_at_recall"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.taoamd_version() >= 101
    # sizes: one layout function, the usual contract
    assert lib.taoamd_score_at_recall_workspace(0, 1, 6) > 0
    small = lib.taoamd_score_at_recall_workspace(1000, 7, 6)
    assert small < lib.taoamd_score_at_recall_workspace(1000, 7, 20) \
        < lib.taoamd_score_at_recall_workspace(100000, 7, 20)
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    args = (1000, 7, 6, p, None, p, p + 8, p, None, p, p, p)
    assert lib.taoamd_score_at_recall(*args, small - 1, None) == 4
    assert lib.taoamd_score_at_recall(1000, 0, 6, *args[3:], small, None) == 2
    assert lib.taoamd_score_at_recall(1000, 7, 6, None, *args[4:], small, None) == 2
