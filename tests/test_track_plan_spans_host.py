"""taoamd_track_iou_plan_spans_host (host only, no GPU): the 3D IoU's launch
plan that keeps track pairs without a common timeline position out of the
tasks.  Every pair is exactly once in a task or on the zero list, the zero list
is exactly what the zero rule defines, the tasks keep the kernel's limits and
hold no row that none of their pairs uses, and taoamd_track_iou_plan_host is
what it was: both functions are held to a restatement of the packing rules in
Python (plan_restated), array for array."""
import types

import numpy as np
import pytest

import spanpop
from test_gpu_parity import _check_plan, _drop_frames
from tao_amodal_amd import engine, flatten as fl
from tao_amodal_amd.synth import synth

TT_ROWS, TT_PAIRS = 32, 64


def plan_restated(f, meta, spans):
    """The packing rules in Python: cells by descending end of timeline
    (stable), a cell's detections by first position (stable), GT blocks of at
    most 31 tracks split evenly, a detection track brings its kept pairs of
    the block, its own row and the rows of their GT tracks where the open task
    lacks them, a
    task is closed when the next track would pass 64 pairs or 32 rows, rows by
    first position (stable).  spans: zero pairs are kept out (the zero rule);
    without, every pair is kept."""
    first, last = meta[:, 0].tolist(), meta[:, 1].tolist()
    d_off, g_off, i_off = (np.asarray(a).tolist() for a in
                           (f.cell_dt_off, f.cell_gt_off, f.cell_iou_off))
    n_dt = d_off[-1]
    tasks, rows_out, pairs_out, out = [], [], [], []
    cur_rows, cur_pairs = [], []            # tracks; (detection track, GT track, place)

    def is_zero(d, g):
        return spans and first[d] <= last[d] and first[g] <= last[g] and \
            (last[d] < first[g] or last[g] < first[d])

    def close():
        if cur_pairs:
            order = sorted(range(len(cur_rows)), key=lambda r: first[cur_rows[r]])
            trk = [cur_rows[r] for r in order]
            tasks.append([len(rows_out), len(trk), len(pairs_out), len(cur_pairs)])
            rows_out.extend(trk)
            for d, g, place in cur_pairs:
                pairs_out.append(trk.index(d) | (trk.index(g) << 8))
                out.append(place)
        del cur_rows[:], cur_pairs[:]
    cells = [c for c in range(len(d_off) - 1)
             if d_off[c + 1] > d_off[c] and g_off[c + 1] > g_off[c]]
    end = {c: max([last[t] for t in range(d_off[c], d_off[c + 1])] +
                  [last[n_dt + t] for t in range(g_off[c], g_off[c + 1])]) for c in cells}
    for c in sorted(cells, key=lambda c: -max(end[c], -1)):
        D, G = d_off[c + 1] - d_off[c], g_off[c + 1] - g_off[c]
        dets = sorted(range(D), key=lambda d: first[d_off[c] + d])
        n_blocks = (G + TT_ROWS - 2) // (TT_ROWS - 1)
        for b in range(n_blocks):
            lo, hi = b * G // n_blocks, (b + 1) * G // n_blocks
            in_task = set()                  # the block's GT tracks that are rows of the open task
            for d in dets:
                td = d_off[c] + d
                kept = [g for g in range(lo, hi) if not is_zero(td, n_dt + g_off[c] + g)]
                if not kept:
                    continue
                fresh = [g for g in kept if g not in in_task]
                if len(cur_pairs) + len(kept) > TT_PAIRS or \
                        len(cur_rows) + len(fresh) + (td not in cur_rows) > TT_ROWS:
                    close()
                    in_task, fresh = set(), kept
                for g in fresh:
                    in_task.add(g)
                    cur_rows.append(n_dt + g_off[c] + g)
                if td not in cur_rows:       # (a row already: its pairs with an earlier block)
                    cur_rows.append(td)
                for g in kept:
                    cur_pairs.append((td, n_dt + g_off[c] + g, i_off[c] + d * G + g))
    close()
    return (np.array(tasks, np.int32).reshape(-1, 4), np.array(rows_out, np.int32),
            np.array(pairs_out, np.int32), np.array(out, np.int64))


def check_spans_plan(f, meta, tasks, rows, pairs, out, zero):
    n_dt = int(f.cell_dt_off[-1])
    n = int(f.cell_iou_off[-1])
    # the zero list is the zero rule's set, each place once
    want_zero = spanpop.zero_places(f, meta)
    assert np.array_equal(np.sort(zero), want_zero)
    assert len(np.unique(zero)) == len(zero)
    # every place exactly once in task_out U zero_out
    seen = np.bincount(np.concatenate([out, zero]), minlength=n)
    assert len(seen) == n and (seen == 1).all()
    _, pd, pg = spanpop.pair_tracks(f)
    for r0, nr, p0, npair in tasks.tolist():
        assert 0 < nr <= TT_ROWS and 0 < npair <= TT_PAIRS
        trk = rows[r0:r0 + nr]
        assert len(set(trk.tolist())) == nr
        assert (np.diff(meta[trk, 0]) >= 0).all()               # by first position
        pr, o = pairs[p0:p0 + npair], out[p0:p0 + npair]
        rd, rg = pr & 0xFF, (pr >> 8) & 0xFF
        assert (pr >> 16 == 0).all() and (rd < nr).all() and (rg < nr).all()
        # each pair's rows are its two tracks
        assert np.array_equal(trk[rd], pd[o]) and np.array_equal(trk[rg], n_dt + pg[o])
        # no row that none of the task's pairs references
        assert set(rd.tolist()) | set(rg.tolist()) == set(range(nr))
    assert int(tasks[:, 1].sum()) == len(rows) and int(tasks[:, 3].sum()) == len(pairs)
    assert len(out) == len(pairs)


def _both_plans(f, meta):
    """Both functions against the restatement; returns the span-aware plan."""
    old = engine.track_iou_plan(f, meta)
    for got, want in zip(old, plan_restated(f, meta, spans=False)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    if hasattr(f, "dt_flags"):
        _check_plan(f, meta, *old)              # "every pair in exactly one task"
    new = engine.track_iou_plan_spans(f, meta)
    check_spans_plan(f, meta, *new)
    for got, want in zip(new[:4], plan_restated(f, meta, spans=True)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert (np.diff(new[4]) > 0).all()          # the zero list in ascending place
    if len(new[4]) == 0:                        # identity when nothing is disjoint
        for a, b in zip(new[:4], old):
            assert np.array_equal(a, b)
    return old, new


@pytest.mark.parametrize("seed,V,F,G,dpf", [(32, 2, 200, 40, 40), (34, 2, 200, 14, 40),
                                            (33, 1, 200, 8, 40), (35, 2, 200, 18, 40)])
def test_spans_plan_on_the_synthetic_sets(seed, V, F, G, dpf):
    gt, dt = synth(seed=seed, V=V, F=F, C=6, dets_per_frame=dpf,
                   gt_tracks_per_video=G, n_present=2, n_neg=1)
    for holes in (False, True):
        if holes:
            gt, dt = _drop_frames(gt, dt, seed)
        dt.track_id, _ = fl.make_track_ids_unique(dt)
        f = fl.flatten_tao(gt, dt)
        meta = engine.track_meta(f)[0]
        old, new = _both_plans(f, meta)
        assert 0 < len(new[4]) < int(f.cell_iou_off[-1])
        assert len(new[0]) < len(old[0]) and len(new[1]) < len(old[1])


@pytest.mark.parametrize("name", list(spanpop.HAND_CELLS))
def test_spans_plan_on_hand_built_cells(name):
    f = spanpop.span_flat(spanpop.HAND_CELLS[name], holes=0.3)
    meta = engine.track_meta(f)[0]
    _, new = _both_plans(f, meta)
    n_zero = {"touching": 0, "adjacent": 2, "nested": 0}.get(name)
    if n_zero is not None:
        assert len(new[4]) == n_zero
    if name == "all_disjoint_cell":
        # the first cell is all zero pairs: none of its tracks is a row
        n_dt = int(f.cell_dt_off[-1])
        c = int(np.flatnonzero(np.diff(f.cell_iou_off) == 9)[0])
        its = set(range(f.cell_dt_off[c], f.cell_dt_off[c + 1])) | \
            set(range(n_dt + f.cell_gt_off[c], n_dt + f.cell_gt_off[c + 1]))
        assert not its & set(new[1].tolist())
    if name == "mixed":
        # LONELY: two detections meet no GT of their cell
        assert int(f.cell_dt_off[-1]) - int((new[1] < f.cell_dt_off[-1]).sum()) == 2


def test_spans_plan_with_every_pair_a_zero_pair():
    f = spanpop.span_flat(spanpop.ALL_ZERO)
    meta = engine.track_meta(f)[0]
    _, new = _both_plans(f, meta)
    assert len(new[0]) == 0 and len(new[1]) == 0 and len(new[2]) == 0
    assert np.array_equal(new[4], np.arange(int(f.cell_iou_off[-1])))


def test_spans_plan_equals_the_old_plan_without_zero_pairs():
    f = spanpop.span_flat(spanpop.no_zero_cells())
    meta = engine.track_meta(f)[0]
    old, new = _both_plans(f, meta)
    assert len(new[4]) == 0 and len(old[0]) > 1
    for a, b in zip(new[:4], old):
        assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("n_gt", [33, 32, 63, 64, 96])
def test_spans_plan_at_the_gt_block_edges(n_gt):
    """40 detection tracks x n_gt GT tracks: one to four GT blocks (the counts
    of test_abi.py's plan test), a fifth of the GTs disjoint from every
    detection, detections that meet no GT; and the same cell without a zero
    pair (every track over the whole timeline)."""
    dts, gts = spanpop.big_cell(n_gt)
    f = spanpop.span_flat([(dts, gts)])
    assert np.diff(f.cell_gt_off).tolist() == [n_gt] and np.diff(f.cell_dt_off).tolist() == [40]
    meta = engine.track_meta(f)[0]
    old, new = _both_plans(f, meta)
    n_dt = 40
    gt_rows = set((new[1][new[1] >= n_dt] - n_dt).tolist())
    zero_gt = set(range(n_gt)) - gt_rows
    assert len(zero_gt) >= n_gt // 5            # GTs behind every detection: rows of no task
    assert len(set(new[1][new[1] < n_dt].tolist())) < 40
    full = [((0, 119),) * 40, ((0, 119),) * n_gt]
    f = spanpop.span_flat([(list(full[0]), list(full[1]))])
    meta = engine.track_meta(f)[0]
    old, new = _both_plans(f, meta)
    assert len(new[4]) == 0 and int(old[0][:, 1].max()) <= TT_ROWS


def test_spans_plan_spills_a_cell_over_several_tasks():
    f = spanpop.span_flat([spanpop.spill_cell(), spanpop.MIXED])
    meta = engine.track_meta(f)[0]
    _, new = _both_plans(f, meta)
    assert len(new[0]) >= 4 and int(new[0][:, 3].max()) > 48


def _hand_meta(cells):
    """(flat-like, trk_meta) of cells given as (detection spans, GT spans); a
    span of None is a track without frames (first = 1, last = 0)."""
    d_off, g_off, i_off, md, mg = [0], [0], [0], [], []
    for dts, gts in cells:
        d_off.append(d_off[-1] + len(dts))
        g_off.append(g_off[-1] + len(gts))
        i_off.append(i_off[-1] + len(dts) * len(gts))
        md += [(1, 0) if s is None else s for s in dts]
        mg += [(1, 0) if s is None else s for s in gts]
    meta = np.zeros((len(md) + len(mg), 4), np.int32)
    meta[:, :2] = np.array(md + mg, np.int32).reshape(-1, 2)
    meta[:len(md), 3] = 1
    f = types.SimpleNamespace(cell_dt_off=np.array(d_off, np.int32),
                              cell_gt_off=np.array(g_off, np.int32),
                              cell_iou_off=np.array(i_off, np.int64), n_cells=len(cells))
    return f, meta


def test_spans_plan_keeps_pairs_of_tracks_without_frames():
    """A track without frames on either side, and on both: no zero pair (the
    reference's 0 / 0 of two empty tracks has to stay), the pair is in a task."""
    cells = [([None, (0, 9), (30, 40)], [(20, 25), None, (0, 3)]),
             ([None], [None]), ([None, None], [(5, 6)]), ([(5, 6)], [None, (7, 9), None]),
             ([], [(0, 3)]), ([(0, 3)], []), ([(0, 3), None], [(4, 5)])]
    f, meta = _hand_meta(cells)
    _, new = _both_plans(f, meta)
    tasks, rows, pairs, out, zero = new
    _, pd, pg = spanpop.pair_tracks(f)
    n_dt = int(f.cell_dt_off[-1])
    empty = (meta[pd, 1] < meta[pd, 0]) | (meta[n_dt + pg, 1] < meta[n_dt + pg, 0])
    assert empty.sum() >= 10 and not np.isin(np.flatnonzero(empty), zero).any()
    assert np.isin(np.flatnonzero(empty), out).all()
    assert len(zero) == 5       # (0,9)x(20,25), (30,40)x(20,25), (30,40)x(0,3), (5,6)x(7,9), (0,3)x(4,5)


def test_spans_plan_sizes_call_and_arguments():
    """The sizes protocol: a first call without buffers gives the four counts;
    the zero list alone can be asked for; NULL tables are refused."""
    from tao_amodal_amd import _lib
    lib = _lib.load()
    assert lib.taoamd_version() >= 104
    f = spanpop.span_flat(spanpop.HAND_CELLS["everything"])
    meta = np.ascontiguousarray(engine.track_meta(f)[0], dtype=np.int32)
    tasks, rows, pairs, out, zero = engine.track_iou_plan_spans(f, meta)
    d_off = np.ascontiguousarray(f.cell_dt_off, dtype=np.int32)
    g_off = np.ascontiguousarray(f.cell_gt_off, dtype=np.int32)
    i_off = np.ascontiguousarray(f.cell_iou_off, dtype=np.int64)
    sizes = np.full(4, -1, np.int64)
    args = (f.n_cells, d_off.ctypes.data, g_off.ctypes.data, i_off.ctypes.data,
            meta.ctypes.data, sizes.ctypes.data)
    only_zero = np.full(len(zero), -1, np.int64)
    assert lib.taoamd_track_iou_plan_spans_host(*args, None, None, None, None,
                                                only_zero.ctypes.data) == 0
    assert sizes.tolist() == [len(tasks), len(rows), len(pairs), len(zero)]
    assert np.array_equal(only_zero, zero)
    assert lib.taoamd_track_iou_plan_spans_host(*args[:5], None, None, None, None, None,
                                                None) == _lib.ERR_ARG
    t = np.zeros((len(tasks), 4), np.int32)
    assert lib.taoamd_track_iou_plan_spans_host(*args, t.ctypes.data, None, None, None,
                                                None) == _lib.ERR_ARG
    # the old function's sizes stay three
    sizes3 = np.full(4, -7, np.int64)
    assert lib.taoamd_track_iou_plan_host(*args[:5], sizes3.ctypes.data, None, None, None,
                                          None) == 0
    assert sizes3[3] == -7 and sizes3[2] == int(f.cell_iou_off[-1])
