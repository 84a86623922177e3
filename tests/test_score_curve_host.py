"""The track-level score thresholds without a GPU: the pass rule's restatement
(tests/score_curve_ref.py) on the special doubles, a layer of the identity on
the hand-written table against brute force, the class layer's host rules (the
best threshold, the default thresholds, the argument validation) and the C
ABI's new symbols and refusals (they come before the first device call)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import identity_ref
import score_curve_ref as ref
from tao_amodal_amd import _lib
from tao_amodal_amd.evaluation.tao_amodal import followers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
TINY = 2.0 ** -1074                   # the least subnormal


def test_pass_rule_on_the_special_doubles():
    below = np.nextafter(0.3, -INF)
    # (score, threshold, passes)
    cases = [(NAN, 0.0, 0), (0.5, NAN, 0), (NAN, NAN, 0), (NAN, -INF, 0),
             (-INF, -INF, 1), (0.0, -INF, 1), (INF, -INF, 1), (INF, INF, 1), (1e308, INF, 0),
             (-INF, 0.0, 0), (-0.0, 0.0, 1), (0.0, -0.0, 1), (TINY, 0.0, 1), (0.0, TINY, 0),
             (TINY, TINY, 1), (-TINY, 0.0, 0), (0.3, 0.3, 1), (below, 0.3, 0), (0.3, below, 1)]
    score = np.array([c[0] for c in cases])
    thr = np.array([[c[1]] for c in cases])              # a layer per case, one category
    got = ref.score_pass(score, np.zeros(len(cases), np.int32), thr)
    assert got.dtype == np.uint8 and got.shape == (len(cases), len(cases))
    assert np.diagonal(got).tolist() == [c[2] for c in cases]
    assert set(np.unique(got).tolist()) <= {0, 1}


def test_pass_rule_on_categories_and_base():
    score = np.array([0.9, 0.9, 0.9, 0.9, 0.1, 0.5])
    cat = np.array([-1, 3, 0, 2, 1, 1], np.int32)        # n_cat = 3: -1 and 3 lie outside
    thr = np.array([[0.0, 0.5, 0.0], [-INF, -INF, -INF], [0.95, 0.05, 0.95]])
    got = ref.score_pass(score, cat, thr)
    assert got.tolist() == [[0, 0, 1, 1, 0, 1], [0, 0, 1, 1, 1, 1], [0, 0, 0, 0, 1, 1]]
    base = np.array([1, 1, 0, 2, 1, 0], np.uint8)        # any value but 0 is "on"
    assert ref.score_pass(score, cat, thr, base).tolist() == \
        [[0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 1, 0], [0, 0, 0, 0, 1, 0]]
    assert ref.score_pass(np.zeros(0), np.zeros(0, np.int32), thr).shape == (3, 0)


# scores on the hand-written table of identity_ref: B, then E, then A fall out
HAND_SCORES = {identity_ref.B: 0.1, identity_ref.E: 0.2, identity_ref.A: 0.3}
HAND_THRS = [0.05, 0.15, 0.25, 0.35]


def _hand():
    f, dt_at, gt_at = identity_ref.hand_flat()
    score = np.full(len(dt_at), 0.9)
    for given, s in HAND_SCORES.items():
        score[dt_at[given]] = s
    f.dt_score = score
    return f, dt_at, gt_at


def test_layers_of_the_identity_on_the_hand_written_table():
    f, dt_at, gt_at = _hand()
    share = identity_ref.share(f, identity_ref.HAND_THR)
    plain = identity_ref.identity_from_share(f, share)
    passed = ref.score_pass(f.dt_score, f.dt_cat, np.repeat(np.array(HAND_THRS)[:, None], 2, 1))
    gone = [sorted(int(np.flatnonzero(dt_at == d)[0]) for d in np.flatnonzero(p == 0))
            for p in passed]
    A, B, E = identity_ref.A, identity_ref.B, identity_ref.E
    assert gone == [[], [B], sorted([B, E]), sorted([A, B, E])]
    layers = [ref.identity_layer(f, share, p) for p in passed]
    assert np.array_equal(layers[0]["cat_counts"], plain["cat_counts"])
    assert np.array_equal(layers[0]["gt_ident"], plain["gt_ident"])
    d_off, g_off = np.asarray(f.cell_dt_off, np.int64), np.asarray(f.cell_gt_off, np.int64)
    for p, got in zip(passed, layers):
        # kept at a layer is kept AND pass; the ground truth's side does not move
        assert np.array_equal(got["kept"], plain["kept"] & (p != 0))
        assert np.array_equal(got["cat_counts"][:, :2], plain["cat_counts"][:, :2])
        assert np.array_equal(got["dt_ident"][p == 0], np.tile([-1, 0], ((p == 0).sum(), 1)))
        for c in range(f.n_cells):
            D, G = d_off[c + 1] - d_off[c], g_off[c + 1] - g_off[c]
            S = share[f.cell_iou_off[c]:f.cell_iou_off[c] + D * G].reshape(D, G)
            W = S[got["kept"][d_off[c]:d_off[c + 1]]][:, got["eligible"][g_off[c]:g_off[c + 1]]]
            assert got["cell_idtp"][c] == identity_ref.brute_force(W), c
        identity_ref.check_assignment(f, got["share"], got, got["gt_ident"], got["dt_ident"])
    counts = np.stack([x["cat_counts"].sum(0) for x in layers])
    assert (counts[:, 1] == counts[0, 1]).all()                        # gt_frames
    assert (np.diff(counts[:, 3]) <= 0).all() and (np.diff(counts[:, 4]) <= 0).all()
    # cell (video 0, category 0): 4 + 4, then A alone takes its greatest share, then nothing
    assert counts[:, 4].tolist() == [11, 8, 5, 0]
    assert counts[:, 2].tolist() == [5, 4, 3, 2]                       # dt_tracks


def test_best_rule():
    thrs = [0.1, 0.2, 0.3, 0.4]
    for values, want in (([1, 3, 3, 2], 1), ([NAN, 0.5, NAN, 0.5], 1), ([NAN] * 4, -1),
                         ([-1, NAN, -1, -2], 0), ([0.0, -0.0, 0.0, NAN], 0), ([], -1),
                         ([-INF, NAN, -INF, NAN], 0)):
        assert followers.best_index(values) == want == ref.best_index(values), values
    b = followers.best_threshold([NAN, 0.5, NAN, 0.5], thrs)
    assert b == {"index": 1, "score_thr": 0.2, "value": 0.5}
    none = followers.best_threshold([NAN] * 4, thrs)
    assert none["index"] == -1 and none["score_thr"] != none["score_thr"]
    assert none["value"] != none["value"]
    per = followers.best_per_category(np.array([[1, NAN, 0.5], [2, NAN, 0.5], [2, NAN, NAN],
                                                [0, NAN, 0.1]]), thrs)
    assert per.dtype == np.float64 and per[:1].tolist() == [0.2] and per[2] == 0.1
    assert np.isnan(per[1])


def test_default_thresholds():
    rng = np.random.default_rng(3)
    score = rng.permutation(np.arange(1, 101) / 100.0)
    got = followers.default_score_thrs(score)
    assert got.dtype == np.float64 and got[0] == 0.01 and len(got) == 10
    assert (np.diff(got) > 0).all() and set(got.tolist()) <= set(score.tolist())
    assert np.array_equal(got, np.quantile(score, np.arange(10) / 10.0, method="lower"))
    # NaN and the infinities take no part; the first is the least finite score
    dirty = np.r_[score, NAN, INF, -INF, NAN]
    assert np.array_equal(followers.default_score_thrs(dirty), got)
    # equal quantiles fold; nothing finite: one threshold every score passes
    assert followers.default_score_thrs([0.5] * 7 + [0.7]).tolist() == [0.5]
    assert followers.default_score_thrs([0.5] * 7 + [0.7] * 3).tolist() == [0.5, 0.7]
    assert followers.default_score_thrs([NAN, INF]).tolist() == [-INF]
    assert followers.default_score_thrs([]).tolist() == [-INF]
    assert np.array_equal(followers.curve_score_thrs(None, dirty), got)


def test_argument_validation():
    assert followers.curve_score_thrs([0.25], []).tolist() == [0.25]
    assert followers.curve_score_thrs([-INF, 0.0, INF], []).tolist() == [-INF, 0.0, INF]
    assert len(followers.curve_score_thrs(np.arange(64) / 64.0, [])) == 64
    for bad in ([], np.arange(65) / 65.0, [0.2, 0.1], [0.1, 0.1], [0.1, NAN], [NAN]):
        with pytest.raises(ValueError, match="score_thrs"):
            followers.curve_score_thrs(bad, [])
    assert followers.curve_measures(("clear", "identity")) == ("identity", "clear")
    assert followers.curve_measures("hota") == ("hota",)
    for bad in ((), ("idf1",), ("hota", "hota"), ("identity", "mota")):
        with pytest.raises(ValueError, match="measures"):
            followers.curve_measures(bad)
    ev = SimpleNamespace(params=SimpleNamespace(cat_ids=[4, 7, 9], use_cats=1), _cat_pos=None)
    assert followers.score_thr_of(ev, None) is None
    assert followers.score_thr_of(ev, 0.5).tolist() == [0.5] * 3
    assert followers.score_thr_of(ev, np.float32(0.5)).dtype == np.float64
    assert followers.score_thr_of(ev, -INF).tolist() == [-INF] * 3
    per = followers.score_thr_of(ev, [0.1, NAN, 0.3])
    assert per[0] == 0.1 and np.isnan(per[1]) and per[2] == 0.3
    for bad in ([0.1, 0.2], [[0.1, 0.2, 0.3]], [], "high", [0.1] * 4):
        with pytest.raises(ValueError, match="score_thr"):
            followers.score_thr_of(ev, bad)
    # params.cat_ids as a subset in another order: the tables' other categories get +inf
    ev._cat_pos = np.array([2, 0])
    ev.flat = SimpleNamespace(cat_ids=np.arange(4))
    got = followers._table_thr(ev, np.array([[0.1, 0.2], [0.3, 0.4]]))
    assert got.tolist() == [[0.2, INF, 0.1, INF], [0.4, INF, 0.3, INF]]


def test_curve_numbers_are_the_single_calls_numbers():
    """curve_numbers forms a row with the functions identity(), hota() and clear()
    form theirs with; here on small integer tables, the best rule on top."""
    rng = np.random.default_rng(8)
    T, K, A = 3, 4, 5
    cc = rng.integers(1, 50, (T, K, 6))
    cc[:, 3] = 0                                          # a category without frames
    cc[..., 4] = np.minimum(cc[..., 4], np.minimum(cc[..., 1], cc[..., 3]))
    tp = np.minimum(rng.integers(0, 50, (T, K, A)), np.minimum(cc[..., 1], cc[..., 3])[..., None])
    loc = tp * (1 << 29)
    ass = np.stack([tp * (1 << 28)] * 3, -1)
    clr = rng.integers(0, 9, (T, K, 7))
    clr[..., 0] = tp[..., 0]
    thrs = np.array([0.1, 0.2, 0.3])
    c = followers.curve_numbers(thrs, cc, tp, loc, ass, clr)
    assert c["cat_counts"].shape == (T, K, 6) and c["cat_counts"].dtype == np.int64
    for name in ("idf1", "hota", "deta", "assa", "mota", "motp", "idsw"):
        assert c[name].shape == (T, K), name
        assert c[name].dtype == (np.int64 if name == "idsw" else np.float64)
    for t in range(T):
        idf1, _, _ = followers.identity_ratios(cc[t, :, 4], cc[t, :, 1], cc[t, :, 3])
        assert np.array_equal(c["idf1"][t], idf1, equal_nan=True)
        r = followers.hota_ratios(tp[t], loc[t], ass[t], cc[t, :, 1:2], cc[t, :, 3:4])
        assert np.array_equal(c["hota"][t][:3], r["hota"].mean(-1)[:3])
        assert np.isnan(c["hota"][t][3]) and np.isnan(c["mota"][t][3])
        full = np.concatenate([cc[t, :, :4], clr[t]], 1)
        assert np.array_equal(c["mota"][t][:3], followers.clear_ratios(full)["mota"][:3])
        assert c["total"]["dt_tracks"][t] == cc[t, :, 2].sum()
        assert c["total"]["dt_frames"][t] == cc[t, :, 3].sum()
        assert c["total"]["mota"][t] == followers.clear_ratios(full.sum(0))["mota"]
    for name, key in (("IDF1", "idf1"), ("HOTA", "HOTA"), ("MOTA", "mota")):
        col = c["total"][key]
        assert col.shape == (T,)
        i = ref.best_index(col)
        assert c["best"][name] == {"index": i, "score_thr": float(thrs[i]), "value": float(col[i])}
        per = c["best_per_category"][name]
        assert per.shape == (K,) and np.isnan(per[3])
        assert per[:3].tolist() == [thrs[ref.best_index(c[name.lower()][:, k])] for k in range(3)]
    lines = followers.curve_lines(dict(c, frame_thr=0.5))
    assert len(lines) == 2 + T and "IDF1" in lines[1] and "IDSW" in lines[1]
    only = followers.curve_numbers(thrs, cc)
    assert set(only["best"]) == {"IDF1"} and "hota" not in only and only["mean"] == {}
    assert "-" in followers.curve_lines(dict(only, frame_thr=0.5))[2]


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    lib = _lib.load()
    for name in ("taoamd_track_score_pass", "taoamd_track_identity_layers_workspace",
                 "taoamd_track_identity_assign_at"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert "track-level score thresholds" in text
    assert lib.taoamd_version() >= 113
    assert _lib.TRACK_SCORE_THRS == 64 == ref.MAX_THRS
    # the layered call: the identity's arguments, n_thr and dt_pass more
    assert len(_lib.SIGNATURES["taoamd_track_identity_assign_at"][1]) == \
        len(_lib.SIGNATURES["taoamd_track_identity_assign"][1]) + 2


def test_abi_refusals_come_before_the_first_device_call():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    n_dt, n_gt, n_gf = 1000, 70, 3000
    one = int(lib.taoamd_track_identity_workspace(n_dt, n_gt, n_gf))
    assert int(lib.taoamd_track_identity_layers_workspace(n_dt, n_gt, n_gf, 1)) == one
    need = int(lib.taoamd_track_identity_layers_workspace(n_dt, n_gt, n_gf, 5))
    # a slice of the search state (40 bytes a row) and of the index lists (4) per layer
    assert need > one and need > 5 * 44 * (n_dt + n_gt)
    for bad in ((-1, n_gt, n_gf, 5), (n_dt, -1, n_gf, 5), (n_dt, n_gt, -1, 5),
                (2 ** 31, n_gt, n_gf, 5), (n_dt, n_gt, n_gf, 0), (n_dt, n_gt, n_gf, 65),
                (n_dt, n_gt, n_gf, -1)):
        assert lib.taoamd_track_identity_layers_workspace(*bad) == 0, bad
    assert lib.taoamd_track_identity_layers_workspace(n_dt, n_gt, n_gf, 64) > need

    def assign(n_cat=7, n_thr=5, sizes=(n_dt, n_gt, 50, 4000, 9000, n_gf), nbytes=need - 1,
               ptrs=None):
        return lib.taoamd_track_identity_assign_at(*sizes, n_cat, n_thr, *(ptrs or [p] * 16),
                                                   nbytes, None)
    assert assign(n_cat=0) == 2 and assign(n_cat=-1) == 2
    assert assign(n_thr=0) == 2 and assign(n_thr=65) == 2 and assign(n_thr=-1) == 2
    for i in range(6):
        sizes = [n_dt, n_gt, 50, 4000, 9000, n_gf]
        sizes[i] = -1
        assert assign(sizes=sizes) == 2, i
    # a missing table: every pointer in turn; gt_ident (the 13th) may be missing
    for i in range(16):
        ptrs = [p] * 16
        ptrs[i] = None
        assert assign(ptrs=ptrs) == (4 if i == 12 else 2), i
    # good arguments, one byte short: the workspace check, still no device call
    assert assign() == 4 and assign(n_thr=1, nbytes=one - 1) == 4 and assign(n_thr=6) == 4

    def passes(n=n_dt, n_cat=3, n_thr=2, ptrs=None):
        return lib.taoamd_track_score_pass(n, n_cat, n_thr, *(ptrs or [p] * 5), None)
    assert passes(n=-1) == 2 and passes(n=2 ** 31) == 2
    assert passes(n_cat=0) == 2 and passes(n_thr=0) == 2 and passes(n_thr=65) == 2
    for i in (0, 1, 2, 4):                               # (base, the 4th, may be missing)
        ptrs = [p] * 5
        ptrs[i] = None
        assert passes(ptrs=ptrs) == 2, i
    # nothing to do is no error, and no launch: only the threshold table is asked for
    assert passes(n=0, ptrs=[None, None, p, None, None]) == 0
    assert passes(n=0, ptrs=[None] * 5) == 2
    assert not buf.any()
