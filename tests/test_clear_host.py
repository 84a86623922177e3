"""Track-level CLEAR without a GPU: the numpy restatement (tests/clear_ref.py) on
the hand-written table with hand-computed expectations, the fixed-point form
against the float64 statement of the definition, the invariants that tie it to
the association and the identity, the class layer's arithmetic on the
restatement's tables, and the C ABI's new symbols and refusals (argument and
workspace checks come before the first device call)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import association_ref
import clear_ref as ref
import hota_ref
from tao_amodal_amd import _lib
from track_error_types_ref import make_track_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ref.ONE

# the seeded population of the host tests: cells of one to four ground truths that
# overlap, real-valued boxes so that no two weights are equal; small enough that
# the float statement can enumerate every step's assignments for the margin
CELLS = [(3, 1), (5, 2), (6, 3), (0, 2), (2, 0), (6, 4), (4, 4), (4, 2), (5, 3)]
SEED = 5
THR = 0.3


@pytest.fixture(scope="module")
def population():
    f = ref.crowded_flat(SEED, CELLS)
    keep = (np.random.default_rng(SEED).random(len(f.dt_cat)) < 0.9).astype(np.uint8)
    rng = np.random.default_rng(SEED + 1)
    vis = rng.choice([0.0, 0.05, 0.1, 0.5, 0.8, 1.0, np.nan], len(f.gt_frame_pos))
    cc, want = ref.table(f, THR, keep, vis, association_ref.VIS_RNG)
    return f, keep, vis, cc, want


def test_restatement_gives_the_hand_numbers():
    f, dt_at, gt_at, keep, vis = ref.hand_flat()
    cc, got = ref.table(f, ref.HAND_THR, keep, vis, ref.HAND_VIS_RNG)
    assert ref.by_given(f, dt_at, gt_at, got["match"], rows=True) == ref.HAND_MATCH
    assert ref.by_given(f, dt_at, gt_at, got["sw"]) == ref.HAND_SW
    assert got["gt_clear"][gt_at].tolist() == ref.HAND_GT_CLEAR
    assert cc.tolist() == ref.HAND_CAT_COUNTS
    assert got["vis_counts"].tolist() == ref.HAND_VIS_COUNTS
    assert ref.ratios(cc)["mota"].tolist() == ref.HAND_MOTA
    assert int(hota_ref.q(0.6)) == ref.Q6
    # (a) the step at which continuity beat IoU: A's 0.6 with the bonus against B's 1.0
    cell = int(f.gt_cell[gt_at[0]])
    st = [s for s in got["steps"] if s[0] == cell and s[1] == 1][0]
    assert st[4].tolist() == [[ref.Q6 + ref.BONUS, ONE]] and st[5] == [0] and st[6] == [(0, 0)]
    # (c) position 1 of video 3 is no step: the bonus is still there at position 2
    cell = int(f.gt_cell[gt_at[3]])
    assert [s[1] for s in got["steps"] if s[0] == cell] == [0, 2]
    assert [s for s in got["steps"] if s[0] == cell][1][4].tolist() == [[ref.Q6 + ref.BONUS, ONE]]
    # (d) both bonuses at the second step of video 4
    cell = int(f.gt_cell[gt_at[4]])
    W = [s for s in got["steps"] if s[0] == cell][1][4]
    assert W.tolist() == [[ref.Q6 + ref.BONUS, ONE], [ONE, ref.Q6 + ref.BONUS]]
    # (h) exactly 0.5 against the threshold 0.5 and the next double
    above, _ = ref.table(f, ref.HAND_THR_ABOVE, keep)
    assert above.tolist() == ref.HAND_CAT_COUNTS_ABOVE
    # a step bit without a candidate (video 2, position 1); none on an ignored frame
    k = int(f.gt_frame_off[gt_at[2]]) + 1
    assert got["step"][k] == 1 and got["cand_off"][k + 1] == got["cand_off"][k]
    k = int(f.gt_frame_off[gt_at[13]])
    assert got["step"][k] == 0 and got["cand_off"][k + 1] == got["cand_off"][k]


def test_fixed_point_against_the_float_statement(population):
    """The restatement and the float statement choose the same pairs at EVERY step
    (asserted, not filtered), so every integer table is equal; MOTP's sum adds one
    q(c(s)) per match, each rounded once by at most 2^-31, so motp_sum / 2^30 / tp
    agrees to 2^-30.  Precondition, asserted on the data: the float optimum of
    every step is unique by more than min(G, D) * 2^-29 -- a weight is off by at
    most 2^-31, an assignment's sum by min(G, D) * 2^-31, the difference of two by
    twice that; the bonus 1000 * 2^30 is exact."""
    pytest.importorskip("scipy.optimize")
    f, keep, vis, cc, want = population
    flt = ref.clear_float(f, THR, keep)
    assert flt["skipped"] == 0 and len(flt["margins"]) > 100
    assert min(flt["margins"]) > 2.0 ** -29
    fixed = {k: v for k, v in ref.fixed_pairs(want, f).items() if v}
    assert fixed == {k: v for k, v in flt["pairs"].items() if v} and len(fixed) > 100
    assert np.array_equal(cc[:, 4:10], flt["cat"]) and cc[:, 4].all() and cc[:, 5].any()
    motp = ref.ratios(cc)["motp"]
    print("motp", np.abs(motp - flt["motp_sum"] / np.maximum(1, cc[:, 4])).max())
    assert np.abs(motp - flt["motp_sum"] / np.maximum(1, cc[:, 4])).max() <= 2.0 ** -30
    # the population holds what it is for: steps of several rows, bonuses at work
    many = [s for s in want["steps"] if len(s[2]) > 1 and len(s[3]) > 1]
    assert len(many) > 50 and sum(any(p >= 0 for p in s[5]) for s in many) > 30
    assert any((s[4] > ref.BONUS).sum() > 1 for s in many)


def test_step_optimum_is_scipys_on_the_integer_matrix(population):
    opt = pytest.importorskip("scipy.optimize")
    for _, _, gf, cols, W, _, pairs, _ in population[4]["steps"]:
        assert len(set(i for i, _ in pairs)) == len(pairs) == len(set(j for _, j in pairs))
        assert W.max() < 2 ** 41 and W.min() >= 0
        r, c = opt.linear_sum_assignment(W, maximize=True)
        assert sum(int(W[i, j]) for i, j in pairs) == int(W[r, c].sum())


def test_invariants(population):
    f, keep, vis, cc, want = population
    assert np.array_equal(cc[:, 4] + (cc[:, 1] - cc[:, 4]), cc[:, 1])
    assert (cc[:, 1] >= cc[:, 4]).all() and (cc[:, 3] - cc[:, 4] >= 0).all()
    assert np.array_equal(cc[:, 7:10].sum(1), cc[:, 0]) and cc[:, 7:10].all(0).any()
    # the windows' frames are the association's, window by window
    assoc = association_ref.association(f, vis, THR)
    assert np.array_equal(want["vis_counts"][..., 0], assoc["vis_counts"][..., 0])
    for w, window in enumerate(association_ref.VIS_RNG):
        one = association_ref.association(f, vis, THR, [window])
        assert np.array_equal(want["vis_counts"][w, :, 0], one["vis_counts"][0, :, 0])
    assert np.isnan(vis).any() and want["vis_counts"][0, :, 0].sum() < cc[:, 1].sum()
    # a one-to-one assignment over fewer tracks matches no more frames than are covered
    assert (cc[:, 4] <= assoc["cat_counts"][:, 2]).all()
    assert (want["vis_counts"][..., 1] <= assoc["vis_counts"][..., 1]).all()
    assert (want["vis_counts"][..., 2] <= want["vis_counts"][..., 1]).all()
    assert want["vis_counts"][..., 2].any()


def test_one_ground_truth_and_disjoint_detections_follow_the_association():
    rng = np.random.default_rng(11)

    def run(lo, hi, dx):
        return {p: [dx + float(rng.normal(0, 0.3)), 0.0, 10.0, 10.0] for p in range(lo, hi)}
    gts = [(0, 0, {p: [0.0, 0.0, 10.0, 10.0] for p in range(30) if p != 17}, 0)]
    dets = [(0, 0, run(0, 10, 0), 0.9, 0), (0, 0, run(12, 21, 2), 0.8, 0),
            (0, 0, run(22, 30, -2), 0.7, 0), (0, 0, run(10, 12, 100), 0.6, 0)]
    f, _, _ = make_track_flat(1, 1, dets, gts)
    vis = np.ones(len(f.gt_frame_pos))
    got = ref.stage(f, 0.5, None)
    assoc = association_ref.association(f, vis, 0.5, [])
    assert np.array_equal(got["match"], assoc["best"])
    assert set(got["match"].tolist()) == {-1, 0, 1, 2}
    assert np.array_equal(got["match_iou"], assoc["best_iou"])
    # positions 10 and 11 are steps without a candidate (prev is lost: started 2);
    # position 21 has no detection frame (no step: prev survives the hole)
    assert got["gt_clear"].tolist() == [[29, 26, 2, 2]]


def _fake_eval(f, keep, vis, seen):
    """An evaluator whose run answers clear_table() with the restatement."""
    f.tl_vid_start = np.arange(len(f.vid_ids), dtype=np.int64) * 1000
    f.tl_image_id = np.arange(len(f.vid_ids) * 1000, dtype=np.int64) + 7

    def clear_table(frame_thr, vis_rng, ann_vis, score_thr=None):
        seen.append((frame_thr, np.array(vis_rng)))
        cc, w = ref.table(f, frame_thr, keep, vis, vis_rng)
        ident = np.zeros((len(f.cat_ids), 6), np.int64)
        ident[:, :4] = cc[:, :4]
        return {"ident_counts": ident, "cat_counts": w["cat_counts"],
                "vis_counts": w["vis_counts"], "gt_clear": w["gt_clear"], "match": w["match"],
                "match_iou": w["match_iou"], "sw": w["sw"]}
    return SimpleNamespace(_run=SimpleNamespace(flat=f, clear_table=clear_table), _cat_pos=None,
                           _clear={}, _gt_columns=SimpleNamespace(ann_vis=None),
                           params=SimpleNamespace(iou_type="bbox"))


def test_class_layer_arithmetic():
    from tao_amodal_amd.evaluation.tao_amodal import followers
    f, dt_at, gt_at, keep, vis = ref.hand_flat()
    f.cat_ids = np.arange(3, dtype=np.int64)            # a third category without frames
    seen = []
    ev = _fake_eval(f, keep, vis, seen)
    e = followers.clear(ev, 0.5, ref.HAND_VIS_RNG, None, False, False)
    assert "tracks" not in e and "frames" not in e and e["frame_thr"] == 0.5
    assert e["cat_counts"].tolist() == ref.HAND_CAT_COUNTS + [[0] * 11]
    assert e["cat_counts"].dtype == np.int64 and e["fn"].tolist() == [2, 11, 0]
    assert e["fp"].tolist() == [4, 3, 0] and e["vis_lbl"] == ["[0, 1]", "[0, 0.5]", "[0.5, 1]"]
    assert e["columns"]["cat_counts"] == list(_lib.IDENT_CAT_COLUMNS[:4]) + list(ref.CAT_COLUMNS)
    r = ref.ratios(np.asarray(ref.HAND_CAT_COUNTS))
    for k in _lib.CLEAR_RATIOS:
        assert e[k].dtype == np.float64 and e[k][:2].tolist() == r[k].tolist(), k
        assert np.isnan(e[k][2])
        assert e["mean"][k] == float(r[k].mean()), k
    assert e["mota"][:2].tolist() == ref.HAND_MOTA
    assert e["motp"][0] == (10 * ONE + 6 * ref.Q6) / ONE / 16
    assert e["mtr"][:2].tolist() == [6 / 8, 2 / 5] and e["mlr"][:2].tolist() == [0.0, 1 / 5]
    assert e["vis_counts"][:, :2].tolist() == ref.HAND_VIS_COUNTS
    assert e["vis_re"][:, 0].tolist() == [15 / 17, 1 / 2, 15 / 16] and np.isnan(e["vis_re"][1, 1])
    tot = e["total"]
    assert [tot[c] for c in ("gt_frames", "dt_frames", "tp", "fn", "fp", "idsw", "frag")] == \
        [41, 35, 28, 13, 7, 1, 2]
    assert tot["mota"] == (28 - 7 - 1) / 41 and tot["clr_re"] == 28 / 41
    assert tot["clr_f1"] == 28 / (56 + 13 + 7) * 2 and tot["mtr"] == 8 / 13
    assert tot["smota"] == ((21 * ONE + ONE // 2 + 6 * ref.Q6) / ONE - 7 - 1) / 41
    # cached per (frame_thr, windows); per_track and per_frame add their tables
    assert followers.clear(ev, 0.5, ref.HAND_VIS_RNG, None, False, False)["fn"] is e["fn"]
    assert len(seen) == 1
    full = followers.clear(ev, 0.5, ref.HAND_VIS_RNG, None, True, True)
    gid, tr = full["tracks"]
    assert np.array_equal(gid, f.gt_id)
    frag = [[a, b, c, max(d - 1, 0)] for a, b, c, d in ref.HAND_GT_CLEAR]
    assert tr[gt_at][:, :4].tolist() == frag
    assert tr[gt_at][:, 4].tolist() == [2, 2, 1, 1, 2, 2, 2, 2, 1, 1, 0, 2, 2, 0, 2]
    gid, img, did, s, sw = full["frames"]
    rows = [k for g in gt_at for k in range(f.gt_frame_off[g], f.gt_frame_off[g + 1])]
    want_ids = [int(f.dt_id[dt_at[m]]) if m >= 0 else -1 for m in ref.HAND_MATCH]
    assert did[rows].tolist() == want_ids and sw[rows].tolist() == ref.HAND_SW
    assert s[rows][:4].tolist() == [0.6, 0.6, 1.0, 1.0] and ((did >= 0) == (s > 0)).all()
    assert len(img) == len(gid) and img.min() >= 7
    followers.clear(ev, 0.5 + 2.0 ** -52, ref.HAND_VIS_RNG, None, False, False)
    assert len(seen) == 2 and len(ev._clear) == 2
    # the default windows are association()'s
    d = followers.clear(ev, 0.5, None, None, False, False)
    assert np.asarray(d["vis_rng"]).tolist() == association_ref.VIS_RNG and len(seen) == 3
    lines = followers.clear_lines(e)
    assert len(lines) == 4 + 3 and lines[1].split()[:4] == ["MOTA", "MOTP", "MODA", "CLR_Re"]
    assert lines[1].split()[-8:] == ["CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag"]
    assert lines[2].split()[0] == "total" and lines[3].split()[:2] == ["class", "mean"]
    assert "{:.2f}".format(100 * tot["mota"]) in lines[2]
    assert lines[2].split()[-8:] == ["28", "13", "7", "1", "8", "4", "1", "2"]
    assert lines[5].split()[-3:] == ["2", "50.00", "1"]


def test_class_layer_value_errors():
    from tao_amodal_amd.evaluation.tao_amodal import followers
    f, _, _, keep, vis = ref.hand_flat()
    ev = _fake_eval(f, keep, vis, [])
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="frame_thr"):
            followers.clear(ev, bad, None, None, False, False)
    with pytest.raises(ValueError, match="vis_rng"):
        followers.clear(ev, 0.5, [[0, 1]] * 9, None, False, False)
    with pytest.raises(ValueError, match="vis_lbl"):
        followers.clear(ev, 0.5, [[0, 1]] * 2, ["a"], False, False)
    assert ev._clear == {}
    ev._run = None
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        followers.clear(ev, 0.5, None, None, False, False)


NAMES = ("taoamd_track_clear_workspace", "taoamd_track_clear_count", "taoamd_track_clear_fill",
         "taoamd_track_clear_walk", "taoamd_track_clear_reduce")


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert lib.taoamd_version() >= 112
    assert _lib.TRACK_CLEAR_BONUS * _lib.HOTA_ONE == ref.BONUS and _lib.TRACK_CLEAR_NMAX == 2 ** 18
    assert _lib.CLEAR_CAT_COLUMNS == ref.CAT_COLUMNS and _lib.CLEAR_VIS_COLUMNS == ref.VIS_COLUMNS
    assert _lib.CLEAR_TRACK_COLUMNS == ref.TRACK_COLUMNS and _lib.CLEAR_RATIOS == ref.RATIOS
    # a weight is below 2^41; three sums of NMAX of them stay below the solver's infinity
    assert ref.BONUS + ONE < 2 ** 41 and 3 * _lib.TRACK_CLEAR_NMAX * 2 ** 41 < 2 ** 61


def test_abi_refusals_come_before_the_first_device_call():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    n_dt, n_gt, n_gf = 1000, 70, 3000
    need = int(lib.taoamd_track_clear_workspace(n_dt, n_gt, n_gf))
    # the frame index, the frames' counts and 80 bytes of state per row
    assert need > 16 * n_dt + 4 * n_gt + 8 * n_gf + 80 * (n_dt + n_gt)
    for bad in ((-1, n_gt, n_gf), (n_dt, -1, n_gf), (n_dt, n_gt, -1), (2 ** 31, n_gt, n_gf)):
        assert lib.taoamd_track_clear_workspace(*bad) == 0
    SIZES = (n_dt, n_gt, 50, 9000, n_gf)

    def count(thr=0.5, sizes=SIZES, nbytes=need - 1, ptrs=None):
        return lib.taoamd_track_clear_count(*sizes, thr, *(ptrs or [p] * 13), nbytes, None)

    def fill(thr=0.5, sizes=SIZES, n_cand=10, nbytes=need - 1, ptrs=None):
        ptrs = ptrs or [p] * 15
        return lib.taoamd_track_clear_fill(*sizes, thr, *ptrs[:11], n_cand, *ptrs[11:14],
                                           ptrs[14], nbytes, None)

    def walk(sizes=(n_dt, n_gt, 50, n_gf, 10), nbytes=need - 1, ptrs=None):
        return lib.taoamd_track_clear_walk(*sizes, *(ptrs or [p] * 16), nbytes, None)

    def reduce(n_cat=7, n_vis=3, sizes=(n_dt, n_gt, n_gf, 10), nbytes=need - 1, ptrs=None):
        return lib.taoamd_track_clear_reduce(*sizes, n_cat, n_vis, *(ptrs or [p] * 14), nbytes,
                                             None)
    for i in range(5):
        sizes = list(SIZES)
        sizes[i] = -1
        assert count(sizes=sizes) == 2 and fill(sizes=sizes) == 2, i
        sizes = [n_dt, n_gt, 50, n_gf, 10]
        sizes[i] = -1
        assert walk(sizes=sizes) == 2, i
    for i in range(4):
        sizes = [n_dt, n_gt, n_gf, 10]
        sizes[i] = -1
        assert reduce(sizes=sizes) == 2, i
    for bad in (0.0, -0.5, 1.0 + 2.0 ** -52, float("nan"), float("inf")):
        assert count(thr=bad) == 2 and fill(thr=bad) == 2, bad
    assert fill(n_cand=-1) == 2
    assert reduce(n_vis=9) == 2 and reduce(n_vis=-1) == 2
    assert reduce(n_cat=0) == 2 and reduce(n_cat=-1) == 2
    # a missing table: every pointer in turn; dt_keep (3), cand_iou and match_iou may
    # be NULL; windows need the visibilities, the windows and their table
    for i in range(13):
        ptrs = [p] * 13
        ptrs[i] = None
        assert count(ptrs=ptrs) == (4 if i == 3 else 2), i
    for i in range(15):
        ptrs = [p] * 15
        ptrs[i] = None
        assert fill(ptrs=ptrs) == (4 if i in (3, 13) else 2), i
    for i in range(16):
        ptrs = [p] * 16
        ptrs[i] = None
        assert walk(ptrs=ptrs) == (4 if i in (8, 11) else 2), i
    for i in range(14):
        ptrs = [p] * 14
        ptrs[i] = None
        assert reduce(ptrs=ptrs) == 2, i
    ptrs = [p] * 14
    ptrs[3] = ptrs[4] = ptrs[12] = None
    assert reduce(ptrs=ptrs) == 2 and reduce(n_vis=0, ptrs=ptrs) == 4
    # good arguments, one byte short: the workspace check, still no device call
    assert count() == 4 and fill() == 4 and walk() == 4 and reduce() == 4
    assert count(thr=1.0) == 4 and count(thr=5e-324) == 4 and reduce(n_vis=8) == 4
