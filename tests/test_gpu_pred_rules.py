"""-m gpu: the prediction-side rules of the table build (tests/predrules.py)
at every edge of csrc/flatten.hip.  Every table comparison is bit for bit
against flatten.py on the same input (through _lvis_both / _tao_both of
test_gpu_flatten.py, which also evaluate the device tables against the C
oracle); flatten.py itself is pinned to the reference's recording on the same
motifs in test_pred_rules_host.py.  The class API is compared with the
recording directly."""
import copy
import json

import numpy as np
import pytest

import predrules
import test_gpu_two_ranks as two
from goldenio import load_eval, load_json_gz, path
from test_gpu_flatten import LVIS_FIELDS, TAO_FIELDS, _lvis_both, _same, _tao_both
from test_pred_rules_host import expand
from tao_amodal_amd import flatten as fl
from tao_amodal_amd.columns import DTColumns

pytestmark = pytest.mark.gpu

# boxes: each side of the 256-thread grids (FL_THREADS), of fl_starts_kernel's
# 1024 threads and of one, two and three 2048-key tiles (FL_TILE)
N_BOXES = [255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6145]
WHERE = ["split", "first", "last"]


def _both(s):
    gt, dt = s.columns()
    _lvis_both(gt, dt, s.max_dets)
    _tao_both(gt, dt, s.max_dets)


@pytest.mark.parametrize("max_dets", [3, 8])
@pytest.mark.parametrize("n", N_BOXES)
def test_box_counts_at_the_grid_and_tile_edges(n, max_dets):
    s = predrules.sized(n, max_dets=max_dets, where=WHERE[n % 3],
                        low_fillers=(n - 200) // 2)
    assert len(s.preds) == n
    _both(s)


@pytest.mark.parametrize("max_dets", [3, 8])
@pytest.mark.parametrize("n_tracks", [255, 256, 257, 2047, 2048, 2049])
def test_track_counts_at_the_grid_and_tile_edges(n_tracks, max_dets):
    # (longer filler tracks, several fillers per image: the cut works on them too)
    s = predrules.sized(n_tracks + 1000, n_tracks=n_tracks, n_images=700, max_dets=max_dets,
                        low_fillers=n_tracks // 3)
    assert len({p["track_id"] for p in s.preds}) == n_tracks
    _both(s)


@pytest.mark.parametrize("max_dets", [3, 8])
@pytest.mark.parametrize("n_images", [1023, 1024, 1025, 2049])
def test_image_counts_each_side_of_the_starts_kernels_threads(n_images, max_dets):
    s = predrules.sized(n_images + 500, n_images=n_images, max_dets=max_dets)
    gt, _ = s.columns()
    assert len(gt.img_id) == n_images
    _both(s)


def _placed(target, max_dets, at=2047):
    """A 2300-box set whose boxes of track `target`, sorted by track id, begin
    at position `at`: as many one-box fillers get ids below the motif tracks'
    as lie between the target's place without any and `at`."""
    s = predrules.sized(2300, max_dets=max_dets, low_fillers=0)
    keys = np.sort([p["track_id"] for p in s.preds])
    s = predrules.sized(2300, max_dets=max_dets,
                        low_fillers=at - int(np.searchsorted(keys, s.tracks[target])))
    return s, np.sort([p["track_id"] for p in s.preds])


@pytest.mark.parametrize("max_dets", [3, 8])
def test_a_doubled_frame_across_the_tile_boundary_of_the_track_keys(max_dets):
    s, keys = _placed("dup_frame.first2", max_dets)
    # the placement, on the host-sorted keys: the track's four boxes (two of
    # them on one image) lie on 2047 | 2048 .. 2050
    assert keys[2046] != keys[2047] and (keys[2047:2051] == s.tracks["dup_frame.first2"]).all()
    _both(s)


@pytest.mark.parametrize("max_dets", [3, 8])
def test_a_tie_group_across_the_tile_boundary_of_the_track_keys(max_dets):
    tie = ["ties.t2", "ties.t4", "ties.t0", "ties.t3", "ties.t1", "ties.mean", "ties.mean"]
    s, keys = _placed(tie[0], max_dets, at=2045)       # (the group's lowest id)
    # the placement, on the host-sorted keys: the group's seven boxes lie on
    # 2045 .. 2047 | 2048 .. 2051, tied tracks of one box on either side of the
    # boundary: a run head on the last key of a tile and on the first of the next
    assert keys[2045:2052].tolist() == [s.tracks[t] for t in tie]
    _both(s)


def test_every_track_id_beyond_2_to_the_40():
    s = predrules.sized(2049, max_dets=3, low_fillers=900)
    for p in s.preds:
        p["track_id"] += 2 ** 40
    _both(s)


def test_only_the_motif_tracks_beyond_2_to_the_31():
    s = predrules.sized(2049, max_dets=8, motif_base=2 ** 31)
    ids = np.array([p["track_id"] for p in s.preds])
    motif = np.array([m != "fill" for m in s.motif])
    assert (ids[~motif] < 2 ** 31).all() and (ids[motif & (ids > 0)] > 2 ** 31).all()
    _both(s)


def test_the_recorded_sets_wide_ids_included():
    for name in predrules.RECORDED:
        _both(predrules.recorded_set(name))


@pytest.mark.parametrize("max_dets", [3, 8])
def test_clash_inputs_are_rejected_where_the_reference_rejects_them(max_dets):
    from tao_amodal_amd import flatten_dev
    rec = load_json_gz("f11", "predrules.json.gz")["m%d" % max_dets]["clash"]
    s = predrules.sized(1025, max_dets=max_dets, wide=True)
    gt, dt = s.columns()
    base = fl.flatten_tao(gt, dt, max_dets)
    clash = predrules.clash_inputs(s)
    for name in ("cat_stay", "vid_cut", "unknown_image"):
        cols = DTColumns.from_json(clash[name])
        message = rec[name]["tao"][1]
        with pytest.raises(flatten_dev.Rejected):
            flatten_dev.flatten_tao_device(gt, cols, "cuda:0", max_dets)
        with pytest.raises(AssertionError) as e:
            flatten_dev.flatten_tao(gt, cols, max_dets, device="cuda:0")
        assert message.startswith(str(e.value)) and len(str(e.value)) >= 40, name
        if name != "unknown_image":         # (a track clash names the track)
            assert " %d " % s.tracks["cut.long"] in str(e.value), name
    cols = DTColumns.from_json(clash["unknown_image"])
    with pytest.raises(AssertionError, match="do not correspond"):
        flatten_dev.flatten_lvis_device(gt, cols, "cuda:0", max_dets)
    with pytest.raises(AssertionError, match="do not correspond"):
        flatten_dev.flatten_lvis(gt, cols, max_dets, device="cuda:0")
    # the category clash that the cut removes: built, and the base set's tracks
    assert rec["cat_cut"]["tao"] is None
    cols = DTColumns.from_json(clash["cat_cut"])
    _tao_both(gt, cols, max_dets)
    got = flatten_dev.flatten_tao_device(gt, cols, "cuda:0", max_dets)
    for k in ("dt_id", "dt_score", "dt_len", "dt_area", "dt_cat", "dt_frame_pos"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(base[k])), k


def test_columns_born_on_the_device(tmp_path, monkeypatch):
    from test_gpu_ingest import device
    from tao_amodal_amd import flatten_dev
    monkeypatch.setattr(DTColumns, "DEVICE_INGEST_MIN_BYTES", 0)
    s = predrules.sized(2049, max_dets=3, low_fillers=900, wide=True)
    gt, dt = s.columns()
    p = str(tmp_path / "pred.json")
    dt.write_json(p)
    born = device(p)
    assert born is not None and getattr(born, "device_columns", None) is not None
    _same(flatten_dev.flatten_tao_device(gt, born, "cuda:0", 3), fl.flatten_tao(gt, dt, 3),
          TAO_FIELDS)
    _same(flatten_dev.flatten_lvis_device(gt, born, "cuda:0", 3), fl.flatten_lvis(gt, dt, 3),
          LVIS_FIELDS)


# ---------------------------------------------------------------------------
# class API
# ---------------------------------------------------------------------------
def test_class_api_on_f11_scores_and_error_types():
    import score_ref
    from test_gpu_scores import _lvis, _scores_of, _tao
    ev = _lvis("f11", "bbox")
    _scores_of(ev, load_eval("f11")["lvis"][0], score_ref.golden_problem("f11", "lvis"))
    assert np.array_equal(ev.eval["recall"], load_eval("f11")["lvis"][1])
    assert ev.error_types() is not None
    ev = _tao("f11")
    _scores_of(ev, load_eval("f11")["tao"][0], score_ref.golden_problem("f11", "tao"))
    assert np.array_equal(ev.eval["recall"], load_eval("f11")["tao"][1])
    want = load_json_gz("f11", "tao.json.gz")["track_scores"]
    assert {str(k): v for k, v in ev.tao_dt.flat.track_scores.items()} == want
    assert ev.tao_dt.flat.required_average


@pytest.mark.parametrize("name", list(predrules.RECORDED))
def test_class_api_under_small_max_dets_equals_the_recording(name, tmp_path):
    from tao_amodal_amd.evaluation.lvis_amodal import LVIS, LVISEval, LVISResults
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval, TaoResults
    from tao_amodal_amd import flatten_dev
    z = np.load(path("f11", "predrules.npz"))
    rec = load_json_gz("f11", "predrules.json.gz")[name]
    s = predrules.recorded_set(name)
    gt_path = str(tmp_path / "gt.json")
    with open(gt_path, "w") as fh:
        json.dump(s.gt, fh)
    gt = LVIS(gt_path)
    ev = LVISEval(gt, LVISResults(gt, copy.deepcopy(s.preds), max_dets=s.max_dets), "bbox")
    ev.evaluate()
    ev.accumulate()
    p, r = expand(z, name + "_lvis")
    assert np.array_equal(ev.eval["precision"], p) and np.array_equal(ev.eval["recall"], r)
    gt = Tao(gt_path)
    preds = copy.deepcopy(s.preds)
    res = TaoResults(gt, preds, max_dets=s.max_dets)
    assert isinstance(res.flat, flatten_dev.DeviceFlat)
    assert {str(k): v for k, v in res.flat.track_scores.items()} == rec["track_scores"]
    assert res.flat.required_average == bool(z[name + "_required_average"])
    assert [q["score"] for q in preds] == z[name + "_tao_score"].tolist()
    assert [q.get("id", 0) for q in preds] == z[name + "_tao_id"].tolist()
    ev = TaoEval(gt, res)
    ev.evaluate()
    ev.accumulate()
    p, r = expand(z, name + "_tao")
    assert np.array_equal(ev.eval["precision"], p) and np.array_equal(ev.eval["recall"], r)


# ---------------------------------------------------------------------------
# two ranks on the one GPU (the harness of test_gpu_two_ranks.py)
# ---------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_both_two_rank_plans_on_the_rule_set(tmp_path):
    # by category, and by video with the `ties` video alone on rank 0: among its
    # own images the tied tracks come in another order than among the images of
    # both ranks (asserted in check_video_plan), so the cell order is right only
    # where the visiting order comes from the whole set (visit_universe).  The
    # ranks' tables and the results equal the single-GPU run; one spawn for both
    two.check_both_plans(tmp_path, 2, "predrules")
