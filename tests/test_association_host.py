"""The track-level association without a GPU: the numpy restatement
(tests/association_ref.py) on the hand-written table with literal expectations,
and the C ABI's new symbols and refusals (argument and workspace checks come
before the first device call)."""
import os
import re

import numpy as np

import association_ref as ref
from tao_amodal_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hand(thr):
    f, dt_at, gt_at, vis = ref.hand_flat()
    return f, dt_at, gt_at, ref.association(f, vis, thr)


def _by_given(got, dt_at, gt_at):
    """gt_assoc in the order the ground truths were given, the primary as the
    number of the detection given."""
    rows = got["gt_assoc"][gt_at].astype(np.int64)
    inv = {int(r): i for i, r in enumerate(dt_at)}
    rows[:, 5] = [inv.get(int(r), -1) for r in rows[:, 5]]
    return rows.tolist()


def test_restatement_reproduces_the_literals():
    f, dt_at, gt_at, got = _hand(ref.HAND_THR)
    assert _by_given(got, dt_at, gt_at) == ref.HAND_ASSOC
    s = int(f.gt_frame_off[gt_at[0]])
    assert got["best"][s:s + 6].tolist() == ref.HAND_BEST_GT0
    assert got["best_iou"][s:s + 6].tolist() == ref.HAND_BEST_IOU_GT0
    # the 6-frame ground truth followed A, A, -, B, A, A
    frames, covered, ids, switches, fragments, primary, primary_frames = ref.HAND_ASSOC[0]
    assert (covered, ids, switches, fragments, primary, primary_frames) == (5, 2, 2, 2, ref.A, 4)
    assert 5 * 4 < 4 * 6 <= 5 * 5            # 4 / 6 is not mostly tracked, 5 / 6 is
    # two detection tracks with identical boxes: the lower row
    assert dt_at[ref.C_] < dt_at[ref.D_] and ref.HAND_ASSOC[1][5] == ref.C_
    # the cell (video 0, category 0): follow in the layout of the IoU matrix
    k = int(f.gt_cell[gt_at[0]])
    assert f.gt_cell[gt_at[4]] == k and gt_at[4] == gt_at[0] + 1
    cell = got["follow"][f.cell_iou_off[k]:f.cell_iou_off[k + 1]].reshape(2, 2)
    assert cell.tolist() == ref.HAND_FOLLOW_CELL0
    assert got["cat_counts"].tolist() == ref.HAND_CAT_COUNTS
    assert got["vis_counts"][:, 0].tolist() == ref.HAND_VIS_COUNTS
    assert not got["vis_counts"][:, 1].any()
    # the ignored ground truth is followed, and counted nowhere: without it the
    # count tables are the same
    assert ref.HAND_ASSOC[4][1] == 2
    for g in range(len(gt_at)):
        col = got["follow"][f.cell_iou_off[f.gt_cell[g]]:f.cell_iou_off[f.gt_cell[g] + 1]]
        G = f.cell_gt_off[f.gt_cell[g] + 1] - f.cell_gt_off[f.gt_cell[g]]
        assert col.reshape(-1, G)[:, g - f.cell_gt_off[f.gt_cell[g]]].sum() == got["gt_assoc"][g, 1]


def test_restatement_at_the_threshold_and_just_above():
    f, dt_at, gt_at, at = _hand(ref.HAND_THR)
    _, _, _, above = _hand(ref.HAND_THR_ABOVE)
    s = int(f.gt_frame_off[gt_at[2]])
    assert at["best_iou"][s] == ref.HAND_THR and at["best"][s] == 0
    assert above["best"][s] == -1 and above["best_iou"][s] == 0.0
    assert _by_given(above, dt_at, gt_at)[2] == ref.HAND_ASSOC_ABOVE_GT2
    assert above["cat_counts"].tolist() == ref.HAND_CAT_COUNTS_ABOVE
    rest = [0, 1, 3, 4]
    assert np.array_equal(above["gt_assoc"][gt_at[rest]], at["gt_assoc"][gt_at[rest]])


def test_restatement_never_takes_another_category():
    """Detection F (category 1) lies on ground truth 2 (category 0) with IoU 1 in
    both frames; were it a candidate, frame 0 (0.5 with E) would be F's."""
    f, dt_at, gt_at, got = _hand(ref.HAND_THR)
    assert f.dt_cat[dt_at[ref.F]] == 1 and f.gt_cat[gt_at[2]] == 0
    assert got["gt_assoc"][gt_at[2], 5] == dt_at[ref.E] and got["gt_assoc"][gt_at[2], 2] == 1


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    assert "#define TAOAMD_TRACK_ASSOCIATION_TILE %d" % _lib.TRACK_ASSOCIATION_TILE in text
    assert "#define TAOAMD_TRACK_ASSOCIATION_VIS %d" % _lib.TRACK_ASSOCIATION_VIS in text
    lib = _lib.load()
    for name in ("taoamd_track_association_workspace", "taoamd_track_association"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name)
    assert lib.taoamd_version() >= 107
    assert _lib.ASSOC_TRACK_COLUMNS == ref.TRACK_COLUMNS and _lib.ASSOC_CAT_COLUMNS == ref.CAT_COLUMNS


def test_abi_refusals_come_before_the_first_device_call():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    n_dt, n_gt, n_gf = 1000, 70, 3000
    need = int(lib.taoamd_track_association_workspace(n_dt, n_gt, n_gf))
    assert need > 16 * n_dt + 4 * n_gt + 4 * n_gf
    assert lib.taoamd_track_association_workspace(-1, n_gt, n_gf) == 0

    def call(frame_thr=0.5, n_vis=5, nbytes=need - 1):
        return lib.taoamd_track_association(
            n_dt, n_gt, 50, 4000, 9000, n_gf, 7, n_vis, frame_thr, *([p] * 20), nbytes, None)
    for bad in (0.0, -0.1, 1 + 2.0 ** -52, float("nan")):
        assert call(frame_thr=bad) == 2, bad
    assert call(n_vis=9) == 2 and call(n_vis=-1) == 2
    # good arguments, one byte short: the workspace check, still no device call
    assert call() == 4 and call(frame_thr=1.0) == 4 and call(frame_thr=2.0 ** -1074) == 4
    assert call(n_vis=0) == 4 and call(n_vis=8) == 4
