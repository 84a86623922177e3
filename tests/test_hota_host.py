"""Track-level HOTA without a GPU: the numpy restatement (tests/hota_ref.py) on
the hand-written table with hand-computed expectations, its per-frame optimum
against scipy on the integer matrix, the fixed-point form against the float64
statement of the paper's formulas, the class layer's arithmetic on the
restatement's tables, and the C ABI's new symbols and refusals (argument and
workspace checks come before the first device call)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import hota_ref as ref
from tao_amodal_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ref.ONE

# the seeded population of the host tests: every cell shape of one to three ground
# truths and a crowd, real-valued boxes so that no two weights are equal
CELLS = [(3, 1), (5, 2), (6, 3), (0, 2), (2, 0), (12, 6), (9, 9)]
LENGTHS = [1, 7, 20, 40]
SEED = 5


@pytest.fixture(scope="module")
def population():
    f = ref.seeded_flat(SEED, CELLS, LENGTHS, timeline=60, real=True)
    keep = (np.random.default_rng(SEED).random(len(f.dt_cat)) < 0.9).astype(np.uint8)
    want = ref.stage(f, ref.HAND_ALPHAS, keep)
    return f, keep, want


def test_restatement_gives_the_hand_numbers():
    f, dt_at, gt_at, keep = ref.hand_flat()
    got = ref.stage(f, ref.HAND_ALPHAS, keep)
    assert ref.match_by_given(f, dt_at, gt_at, got["match"]) == ref.HAND_MATCH
    iou = [float(got["match_iou"][k]) for g in gt_at
           for k in range(f.gt_frame_off[g], f.gt_frame_off[g + 1])]
    assert iou == ref.HAND_MATCH_IOU
    assert got["tp"].tolist() == ref.HAND_TP
    assert ref.frame_counts(f, keep).tolist() == ref.HAND_COUNTS
    assert got["ass"][:, :, 0].tolist() == ref.HAND_ASS0
    # a set-aside or ignored row has no alignment at all
    G = np.diff(f.cell_gt_off)
    for d in dt_at[ref.HAND_SET_ASIDE]:
        k = int(f.dt_cell[d])
        row = f.cell_iou_off[k] + (d - f.cell_dt_off[k]) * G[k]
        assert not got["pot"][row:row + G[k]].any()
    cnt = np.asarray(ref.HAND_COUNTS)
    r = ref.ratios(got["tp"], got["loc"], got["ass"], cnt[:, 1:2], cnt[:, 3:4])
    assert r["deta"].tolist() == ref.HAND_DETA and r["assa"].tolist() == ref.HAND_ASSA
    # the paper's example: TP = 4, DetA = 1, AssA = 0.5, HOTA = sqrt(0.5)
    assert (r["hota"][0] == ref.HAND_HOTA0).all() and (r["loca"][0] == 1.0).all()
    assert (r["assre"][0] == 0.5).all() and (r["asspr"][0] == 1.0).all()
    # greedy by s would have taken (C, 1): the frame's optimum differs
    grp = [g for g in got["groups"] if g[0] == int(f.gt_cell[gt_at[1]])]
    assert len(grp) == 1 and sorted(grp[0][5]) == [(0, 1), (1, 0)]
    W = grp[0][4]
    assert W[0, 0] == W.max() and W[0, 1] + W[1, 0] > W[0, 0] and W[1, 1] == 0
    # exactly 0.5 against alpha = 0.5 and the next double
    for alpha, tp in ((0.5, ref.HAND_TP_AT_HALF), (0.5 + 2.0 ** -52, ref.HAND_TP_ABOVE_HALF)):
        assert ref.stage(f, [alpha], keep)["tp"].tolist() == tp


def test_frame_optimum_is_scipys_on_the_integer_matrix(population):
    opt = pytest.importorskip("scipy.optimize")
    f, keep, want = population
    many = 0
    for _, _, gf, dl, W, pairs, _ in want["groups"]:
        assert len(set(i for i, _ in pairs)) == len(pairs) == len(set(j for _, j in pairs))
        assert W.size == 0 or (W.max() <= ONE and W.min() >= 0)
        r, c = opt.linear_sum_assignment(W, maximize=True) if W.size else ([], [])
        assert sum(int(W[i, j]) for i, j in pairs) == int(W[r, c].sum()) if W.size else not pairs
        many += len(gf) > 1 and len(dl) > 1
    assert many > 50 and len(want["groups"]) > 150


def test_fixed_point_against_the_float_statement(population):
    """The seed is chosen so that both forms choose the same pairs on EVERY frame
    (asserted, not filtered).  Then tp is equal and every ratio agrees to 2^-30:
    a fixed-point term is off by at most 2^-31 (half a unit of 2^-30), a ratio
    divides at most TP such terms by max(1, TP), and float64's own rounding of
    the float side is orders below.  HOTA = sqrt(DetA * AssA) moves by
    dAssA * DetA / (2 HOTA)."""
    pytest.importorskip("scipy.optimize")
    f, keep, want = population
    flt = ref.hota_float(f, ref.HAND_ALPHAS, keep)
    fixed = ref.fixed_pairs(want)
    assert fixed.keys() == flt["pairs"].keys()
    assert all(fixed[k] == flt["pairs"][k] for k in fixed)
    assert np.array_equal(want["tp"], flt["tp"]) and want["tp"].min() >= 0 and want["tp"].any()
    cnt = ref.frame_counts(f, keep)
    r = ref.ratios(want["tp"], want["loc"], want["ass"], cnt[:, 1:2], cnt[:, 3:4])
    bound = 2.0 ** -30
    for k in ("deta", "detre", "detpr", "assa", "assre", "asspr", "loca"):
        print(k, float(np.abs(r[k] - flt[k]).max()))
        assert np.abs(r[k] - flt[k]).max() <= bound, k
    with np.errstate(all="ignore"):
        room = np.where(flt["hota"] > 0, 2.0 ** -31 * flt["deta"] / (2 * flt["hota"]), 0) + 1e-15
    print("hota", float(np.abs(r["hota"] - flt["hota"]).max()))
    assert (np.abs(r["hota"] - flt["hota"]) <= np.maximum(room, 0)).all()
    assert (flt["assa"] > 0).any() and (flt["assa"] < 1).any()


def _fake_eval(f, keep, alphas_seen):
    """An evaluator whose run answers hota_table() with the restatement."""
    f.tl_vid_start = np.arange(len(f.vid_ids), dtype=np.int64) * 1000
    f.tl_image_id = np.arange(len(f.vid_ids) * 1000, dtype=np.int64) + 7

    def hota_table(alphas, frame_thr, score_thr=None):
        alphas_seen.append(np.array(alphas))
        w = ref.stage(f, alphas, keep)
        cc = np.zeros((len(f.cat_ids), 6), np.int64)
        cc[:, :4] = ref.frame_counts(f, keep)
        return {"cat_counts": cc, "tp": w["tp"], "loc": w["loc"], "ass": w["ass"],
                "match": w["match"], "match_iou": w["match_iou"]}
    return SimpleNamespace(_run=SimpleNamespace(flat=f, hota_table=hota_table), _cat_pos=None,
                           _hota={})


def test_class_layer_arithmetic():
    from tao_amodal_amd.evaluation.tao_amodal import followers
    f, dt_at, gt_at, keep = ref.hand_flat()
    f.cat_ids = np.arange(3, dtype=np.int64)            # a third category without frames
    seen = []
    ev = _fake_eval(f, keep, seen)
    e = followers.hota(ev, None, 0.5, False)
    assert np.array_equal(seen[0], ref.DEFAULT_ALPHAS - np.finfo(float).eps)
    assert np.array_equal(e["alphas"], ref.DEFAULT_ALPHAS) and "frames" not in e
    assert e["cat_counts"].tolist() == ref.HAND_COUNTS + [[0, 0, 0, 0]]
    tp = np.asarray(ref.HAND_TP + [[0] * 19])
    assert np.array_equal(e["tp"], tp)
    assert np.array_equal(e["fn"], e["cat_counts"][:, 1:2] - tp)
    assert np.array_equal(e["fp"], e["cat_counts"][:, 3:4] - tp)
    assert e["deta"][:2].tolist() == ref.HAND_DETA and e["assa"][:2].tolist() == ref.HAND_ASSA
    assert (e["hota"][0] == ref.HAND_HOTA0).all()
    # neither ground-truth nor detection frames: NaN, and outside the class mean
    for k in _lib.HOTA_RATIOS:
        assert e[k].shape == (3, 19) and e[k].dtype == np.float64
        assert np.isnan(e[k][2]).all() and not np.isnan(e[k][:2]).any(), k
    # the total: sums, then ratios; TP = 8 of 8 + 11 frames at the low alphas
    tot = e["total"]
    assert [tot[c] for c in ("gt_tracks", "gt_frames", "dt_tracks", "dt_frames")] == [4, 8, 6, 11]
    assert tot["tp"].tolist() == [8] * 10 + [5] * 9 and tot["fn"].tolist() == [0] * 10 + [3] * 9
    assert tot["fp"].tolist() == [3] * 10 + [6] * 9
    assert tot["deta"].tolist() == [8 / 11] * 10 + [5 / 14] * 9
    assert tot["assa"][0] == (2 + 4) / 8 and tot["assa"][-1] == (2 * ONE + 357913941) / ONE / 5
    assert tot["HOTA"] == float(np.sqrt(tot["deta"] * tot["assa"]).mean())
    assert tot["HOTA(0)"] == float(np.sqrt(8 / 11 * 0.75)) and tot["LocA(0)"] == tot["loca"][0]
    assert tot["HOTALocA(0)"] == tot["HOTA(0)"] * tot["LocA(0)"]
    # the class mean: the per-category means over alpha, over the two with frames
    for name in followers.HOTA_SCALARS:
        per = e[name.lower()][:2].mean(1)
        assert e["mean"][name] == float(per.mean()), name
    assert e["mean"]["HOTA(0)"] == float(e["hota"][:2, 0].mean())
    # cached per (alphas, frame_thr); per_frame adds the frames
    assert followers.hota(ev, None, 0.5, False)["tp"] is e["tp"] and len(seen) == 1
    full = followers.hota(ev, None, 0.5, True)
    gid, img, did, s = full["frames"]
    rows = [k for g in gt_at for k in range(f.gt_frame_off[g], f.gt_frame_off[g + 1])]
    want_ids = [int(f.dt_id[dt_at[m]]) if m >= 0 else -1 for m in ref.HAND_MATCH]
    assert did[rows].tolist() == want_ids and s[rows].tolist() == ref.HAND_MATCH_IOU
    assert gid[rows].tolist() == [int(f.gt_id[g]) for g in gt_at
                                  for _ in range(f.gt_frame_off[g], f.gt_frame_off[g + 1])]
    assert len(img) == len(gid) and img.min() >= 7
    followers.hota(ev, [0.5], 0.5, False)
    assert len(seen) == 2 and len(ev._hota) == 2
    lines = followers.hota_lines(e)
    assert len(lines) == 4 and "HOTA" in lines[1] and "HOTALocA(0)" in lines[1]
    assert lines[2].split()[0] == "total" and lines[3].split()[:2] == ["class", "mean"]
    assert "{:.2f}".format(100 * tot["HOTA"]) in lines[2]


def test_class_layer_value_errors():
    from tao_amodal_amd.evaluation.tao_amodal import followers
    f, _, _, keep = ref.hand_flat()
    ev = _fake_eval(f, keep, [])
    for bad in ([], [0.0, 0.5], [0.5, 1.0 + 2.0 ** -52], [0.5, 0.5], [0.6, 0.5],
                [float("nan")], np.linspace(0.01, 0.99, 33)):
        with pytest.raises(ValueError, match="alphas"):
            followers.hota(ev, bad, 0.5, False)
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="frame_thr"):
            followers.hota(ev, None, bad, False)
    assert ev._hota == {}
    assert len(followers.hota_alphas(np.linspace(0.01, 0.99, 32))) == 32
    ev._run = None
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        followers.hota(ev, None, 0.5, False)


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    lib = _lib.load()
    for name in ("taoamd_track_hota_workspace", "taoamd_track_hota_align",
                 "taoamd_track_hota_match", "taoamd_track_hota_reduce"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert lib.taoamd_version() >= 111
    assert _lib.HOTA_ONE == ONE == 2 ** 30 and _lib.TRACK_HOTA_ALPHAS == 32
    assert _lib.HOTA_RATIOS == ref.RATIOS


def test_abi_refusals_come_before_the_first_device_call():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    n_dt, n_gt, n_gf = 1000, 70, 3000
    need = int(lib.taoamd_track_hota_workspace(n_dt, n_gt, n_gf))
    # the frame index, gt_meta and 48 bytes of group state per row
    assert need > 16 * n_dt + 20 * n_gt + 4 * n_gf + 48 * (n_dt + n_gt)
    for bad in ((-1, n_gt, n_gf), (n_dt, -1, n_gf), (n_dt, n_gt, -1), (2 ** 31, n_gt, n_gf)):
        assert lib.taoamd_track_hota_workspace(*bad) == 0
    good = np.array([0.25, 0.5, 0.75])
    SIZES = (n_dt, n_gt, 50, 4000, 9000, n_gf)

    def align(sizes=SIZES, nbytes=need - 1, ptrs=None):
        return lib.taoamd_track_hota_align(*sizes, *(ptrs or [p] * 13), nbytes, None)

    def match(alphas=good, n_alpha=None, sizes=SIZES, nbytes=need - 1, ptrs=None):
        a = np.ascontiguousarray(alphas, np.float64)
        return lib.taoamd_track_hota_match(*sizes, len(a) if n_alpha is None else n_alpha,
                                           a.ctypes.data if len(a) else None,
                                           *(ptrs or [p] * 18), nbytes, None)

    def reduce(n_cat=7, n_alpha=3, sizes=SIZES, nbytes=need - 1, ptrs=None):
        return lib.taoamd_track_hota_reduce(*sizes, n_cat, n_alpha, *(ptrs or [p] * 13), nbytes,
                                            None)
    for i in range(6):
        sizes = list(SIZES)
        sizes[i] = -1
        assert align(sizes=sizes) == 2 and match(sizes=sizes) == 2 and reduce(sizes=sizes) == 2, i
    for bad in ([0.5, 0.5], [0.5, 0.25], [0.5, float("nan")], [float("nan")], []):
        assert match(alphas=bad) == 2, bad
    assert match(alphas=np.linspace(0.1, 0.9, 33)) == 2 and match(n_alpha=0) == 2
    assert reduce(n_alpha=0) == 2 and reduce(n_alpha=33) == 2
    assert reduce(n_cat=0) == 2 and reduce(n_cat=-1) == 2
    # a missing table: every pointer in turn; dt_keep (align 4, match 4) and
    # match_iou (match 15) may be NULL
    for i in range(13):
        ptrs = [p] * 13
        ptrs[i] = None
        assert align(ptrs=ptrs) == (4 if i == 4 else 2), i
        assert reduce(ptrs=ptrs) == 2, i
    for i in range(18):
        ptrs = [p] * 18
        ptrs[i] = None
        assert match(ptrs=ptrs) == (4 if i in (4, 15) else 2), i
    # good arguments, one byte short: the workspace check, still no device call
    assert align() == 4 and reduce() == 4 and reduce(n_alpha=32) == 4
    assert match() == 4 and match(alphas=np.linspace(0.1, 0.9, 32)) == 4 and match([0.5]) == 4
