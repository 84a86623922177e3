"""The score at each recall threshold, restated in numpy from the reference's
accumulate (lvis_amodal/eval.py:382-417 == tao_amodal/eval.py:538-573) and
pycocotools' ``ss[ri] = dtScoresSorted[pi]``: for one (category, range) the
reference computes ``rec_thrs_insert_idx = np.searchsorted(rc, rec_thrs,
side="left")`` and reads the precision envelope there under a bare ``except``;
the score table reads the sorted scores at the same index under the same
``except``.  Also: the golden tables of a fixture in the form the restatement
takes, shared by the host and the GPU tests."""
import functools

import numpy as np

from goldenio import load_json_gz


def insert_index(tp_row, num_gt, rec_thrs):
    """rec_thrs_insert_idx of one IoU threshold (L/eval.py:383-386,406-408)."""
    tp = np.cumsum(tp_row).astype(dtype=float)
    rc = tp / num_gt
    return np.searchsorted(rc, rec_thrs, side="left")


def score_at_recall(tps, dt_scores, num_gt, rec_thrs):
    """scores[T, R] of one (category, range) with num_gt > 0: tps[T, N] bool in
    the sweep's order, dt_scores[N] sorted the same way."""
    dt_scores = np.asarray(dt_scores, dtype=np.float64)
    out = np.zeros((len(tps), len(rec_thrs)))
    for t, row in enumerate(tps):
        idx = insert_index(row, num_gt, rec_thrs)
        try:
            for j, pi in enumerate(idx):
                out[t, j] = dt_scores[pi]
        except IndexError:
            pass
    return out


def precision_at_recall(tps, fps, num_gt, rec_thrs):
    """The reference's precision[T, R] of the same (category, range), read at
    insert_index() (L/eval.py:382-417): what pins the index to the goldens."""
    out = np.zeros((len(tps), len(rec_thrs)))
    for t, (tp_row, fp_row) in enumerate(zip(tps, fps)):
        tp = np.cumsum(tp_row).astype(dtype=float)
        fp = np.cumsum(fp_row).astype(dtype=float)
        pr = (tp / (fp + tp + np.spacing(1))).tolist()
        for i in range(len(tp) - 1, 0, -1):
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        idx = insert_index(tp_row, num_gt, rec_thrs)
        try:
            for j, pi in enumerate(idx):
                out[t, j] = pr[pi]
        except IndexError:
            pass
    return out


def table(problem, shape, rec_thrs, precision=False):
    """[T, R, K, n_rng] from {(k, a): (tps, fps, scores, num_gt)}: -1 where the
    reference leaves the (category, range) out."""
    out = -np.ones(shape)
    for (k, a), (tps, fps, scores, num_gt) in problem.items():
        out[:, :, k, a] = precision_at_recall(tps, fps, num_gt, rec_thrs) if precision \
            else score_at_recall(tps, scores, num_gt, rec_thrs)
    return out


@functools.lru_cache(maxsize=None)
def golden_problem(name, side):
    """{(k, a): (tps[T, N], fps[T, N], dt_scores[N], num_gt)} of a fixture's
    recorded reference run (``lvis.json.gz`` / ``tao.json.gz``): tps / fps and
    the order of the detections from ``dt_pointers``, their scores from the
    per-cell ``dt_ids`` / ``dt_scores``, num_gt from the per-cell ``gt_ignore``
    (L/eval.py:363-365).  a = the flat range index.  Read-only."""
    want = load_json_gz(name, side + ".json.gz")
    cat_of = {c: k for k, c in enumerate(want["cat_ids"])}
    n_rng = len(want["cells"][0]["ranges"])
    num_gt = np.zeros((len(cat_of), n_rng), dtype=np.int64)
    score_of = {}
    for cell in want["cells"]:
        k = cat_of[cell["key"][1]]
        for a, e in enumerate(cell["ranges"]):
            num_gt[k, a] += int(np.count_nonzero(np.asarray(e["gt_ignore"]) == 0))
            for i, s in zip(e["dt_ids"], e["dt_scores"]):
                seen = score_of.setdefault(int(i), s)
                assert seen == s or (seen != seen and s != s)      # (a NaN score)
    out = {}
    for p in want["dt_pointers"]:
        k, a = p["idx"][0], p["idx"][1]
        if len(p["idx"]) == 3:
            a = a * 4 + p["idx"][2]
        ids = [int(i) for i in p["dt_ids"]]
        # (the reference's ten IoU thresholds; a category may have no detections)
        tps = np.asarray(p["tps"], dtype=bool).reshape(10, len(ids))
        fps = np.asarray(p["fps"], dtype=bool).reshape(10, len(ids))
        scores = np.asarray([score_of[i] for i in ids], dtype=np.float64)
        assert num_gt[k, a] > 0
        for arr in (tps, fps, scores):
            arr.setflags(write=False)
        out[k, a] = (tps, fps, scores, int(num_gt[k, a]))
    return out


def pointers_problem(ev, scores_by_id, n_rng, n_time=None):
    """The same form from an evaluator's own eval["dt_pointers"] (fixtures whose
    goldens hold the tables only): the caller pins it to the golden precision
    with precision_at_recall()."""
    out = {}
    ptr = ev.eval["dt_pointers"]
    run = ev._run
    ng = run.ws.num_gt.cpu().numpy()
    if ev._cat_pos is not None:
        ng = ng[ev._cat_pos]
    for k in range(len(ptr)):
        for a in range(n_rng):
            leaf = ptr[k][a] if n_time is None else ptr[k][a // n_time][a % n_time]
            if not leaf:
                continue
            out[k, a] = (leaf["tps"], leaf["fps"],
                         np.asarray([scores_by_id[int(i)] for i in leaf["dt_ids"]],
                                    dtype=np.float64), int(ng[k, a]))
    return out
