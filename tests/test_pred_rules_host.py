"""The prediction-side rules of the table build (tests/predrules.py) on the
host: flatten.py, the Python oracle and the class API's list rewrite against
what the reference's class API did with the same sets under max_dets 3 and 8
(tests/golden/f11/predrules.npz, recorded by make_golden_predrules.py).
flatten.py is the expectation of the device build in test_gpu_pred_rules.py;
this file pins it to the reference first."""
import copy
import json

import numpy as np
import pytest

import orclib
import predrules
from goldenio import load_json_gz, path
from oracle import pyoracle
from tao_amodal_amd import flatten as fl
from tao_amodal_amd.columns import DTColumns
from tao_amodal_amd.evaluation.lvis_amodal import LVIS, LVISResults
from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoResults

SETS = list(predrules.RECORDED)


@pytest.fixture(scope="module")
def recording():
    return np.load(path("f11", "predrules.npz")), load_json_gz("f11", "predrules.json.gz")


def expand(z, key):
    """(precision, recall) of the recording, the all -1 categories put back."""
    shape = tuple(int(x) for x in z[key + "_shape"])
    k = z[key + "_valid_k"]
    p = -np.ones(shape)
    p[:, :, k] = z[key + "_precision"]
    r = -np.ones((shape[0],) + shape[2:])
    r[:, k] = z[key + "_recall"]
    return p, r


@pytest.mark.parametrize("name", SETS)
def test_sets_hold_what_they_name(name, recording):
    z, j = recording
    s = predrules.recorded_set(name)
    # by the reference's word, and by flatten.py's (which the larger sets of
    # the GPU tests are checked with)
    predrules.check_situations(
        s, predrules.Outcome.from_recording(z[name + "_tao_post_cut"], j[name]))
    gt, dt = s.columns()
    predrules.check_situations(s, predrules.Outcome.from_flat(
        fl.limit_dets_per_image(dt, s.max_dets), fl.flatten_tao(gt, dt, s.max_dets)))
    f = fl.flatten_tao(gt, dt, s.max_dets)
    assert (np.asarray(f.dt_len) != np.diff(np.asarray(f.dt_frame_off))).sum() >= 4


def test_padded_sets_hold_what_they_name():
    for kw in (dict(n_boxes=2049, max_dets=3), dict(n_boxes=400, n_tracks=257, n_images=100,
                                                    max_dets=8, where="first")):
        s = predrules.sized(**kw)
        gt, dt = s.columns()
        assert len(dt) == kw["n_boxes"] and s.motif[0] != "fill"
        assert len(np.unique(dt.track_id)) == kw.get("n_tracks", len(np.unique(dt.track_id)))
        assert len(gt.img_id) == kw.get("n_images", len(gt.img_id))
        predrules.check_situations(s, predrules.Outcome.from_flat(
            fl.limit_dets_per_image(dt, s.max_dets), fl.flatten_tao(gt, dt, s.max_dets)))


@pytest.mark.parametrize("name", SETS)
def test_flatten_and_oracles_equal_the_recorded_class_api(name, recording, monkeypatch):
    z, j = recording
    rec = j[name]
    s = predrules.recorded_set(name)
    m = s.max_dets
    gt, dt = s.columns()
    entered = []
    unique_frames = fl._unique_frames
    monkeypatch.setattr(fl, "_unique_frames",
                        lambda *a: entered.append(1) or unique_frames(*a))
    # ---- the cut: list order, ids
    for side in ("lvis", "tao"):
        assert fl.limit_dets_per_image(dt, m).tolist() == z[name + "_%s_post_cut" % side].tolist()
    fL = fl.flatten_lvis(gt, dt, m)
    assert np.array_equal(z[name + "_lvis_id"][fL.dt_row], fL.dt_id)
    assert np.array_equal(z[name + "_lvis_area"][fL.dt_row],
                          dt.bbox[fL.dt_row, 2] * dt.bbox[fL.dt_row, 3])
    f = fl.flatten_tao(gt, dt, m)
    # the set has tracks with two boxes on an image: not the fast path of track_frames
    assert entered, "the else branch of track_frames was not entered"
    # ---- tracks: score, len, area, frames, the box kept per frame
    assert {str(t) for t in f.dt_id.tolist()} == set(rec["tracks"])
    off = np.asarray(f.dt_frame_off)
    pos, ann = np.asarray(f.dt_frame_pos), np.asarray(f.dt_frame_ann)
    box = np.asarray(f.dt_frame_box)
    for i, t in enumerate(f.dt_id.tolist()):
        r = rec["tracks"][str(t)]
        v = int(np.searchsorted(f.vid_ids, r["video_id"]))
        assert f.vid_ids[v] == r["video_id"] == f.vid_ids[f.cell_unit[f.dt_cell[i]]]
        assert f.cat_ids[f.dt_cat[i]] == r["category_id"]
        assert float(f.dt_score[i]) == r["score"], t
        assert int(f.dt_len[i]) == r["len"], t
        assert float(f.dt_area[i]) == r["area"], t
        ims = f.tl_image_id[f.tl_vid_start[v] + pos[off[i]:off[i + 1]]]
        assert ims.tolist() == r["frame_images"], t
        assert ann[off[i]:off[i + 1]].tolist() == r["frame_boxes"], t
        assert np.array_equal(box[off[i]:off[i + 1]], dt.bbox[r["frame_boxes"]]), t
    assert {str(k): v for k, v in f.track_scores.items()} == rec["track_scores"]
    assert f.required_average == bool(z[name + "_required_average"])
    # ---- cell order
    cells = {(int(f.vid_ids[u]), int(f.cat_ids[c])): k
             for k, (u, c) in enumerate(zip(f.cell_unit, f.cell_cat))}
    for c in rec["cells"]:
        k = cells[tuple(c["key"])]
        assert f.dt_id[f.cell_dt_off[k]:f.cell_dt_off[k + 1]].tolist() == c["dt_ids"], c["key"]
    assert sum(len(c["dt_ids"]) for c in rec["cells"]) == len(f.dt_id)
    # ---- precision / recall: C oracle on flatten.py's tables, Python oracle
    for side, flat in (("lvis", fL), ("tao", f)):
        p, r = expand(z, name + "_" + side)
        out = orclib.run_flat(flat, detail=False)
        assert np.array_equal(out["precision"].reshape(p.shape), p), side
        assert np.array_equal(out["recall"].reshape(r.shape), r), side
    py = pyoracle.lvis_eval(s.gt, s.preds, max_dets=m)
    p, r = expand(z, name + "_lvis")
    assert np.array_equal(py["precision"], p) and np.array_equal(py["recall"], r)
    py = pyoracle.tao_eval(s.gt, s.preds, max_dets=m)
    p, r = expand(z, name + "_tao")
    assert np.array_equal(py["precision"], p) and np.array_equal(py["recall"], r)
    assert {str(k): v for k, v in py["track_scores"].items()} == rec["track_scores"]


@pytest.mark.parametrize("name", SETS)
def test_clash_inputs_raise_what_the_reference_raises(name, recording, tmp_path):
    rec = recording[1][name]["clash"]
    s = predrules.recorded_set(name)
    gt, dt = s.columns()
    want = fl.flatten_tao(gt, dt, s.max_dets)
    gt_path = str(tmp_path / "gt.json")
    with open(gt_path, "w") as fh:
        json.dump(s.gt, fh)
    assert rec["cat_cut"] == {"lvis": None, "tao": None}
    assert [rec[c]["tao"][0] for c in ("cat_stay", "vid_cut", "unknown_image")] == \
        ["AssertionError"] * 3
    for cname, preds in predrules.clash_inputs(s).items():
        cols = DTColumns.from_json(preds)
        for side, build, api in (
                ("lvis", lambda: fl.flatten_lvis(gt, cols, s.max_dets),
                 lambda: LVISResults(LVIS(gt_path), copy.deepcopy(preds), max_dets=s.max_dets)),
                ("tao", lambda: fl.flatten_tao(gt, cols, s.max_dets),
                 lambda: TaoResults(Tao(gt_path), copy.deepcopy(preds), max_dets=s.max_dets))):
            if rec[cname][side] is None:
                got = build()
                api()
                if side == "tao":       # the clash went with the cut: the base set's tables
                    for k in ("dt_id", "dt_score", "dt_len", "dt_area", "dt_cat",
                              "dt_frame_off", "dt_frame_pos"):
                        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
                continue
            kind, message = rec[cname][side]
            assert kind == "AssertionError"
            with pytest.raises(AssertionError) as e:
                build()
            # (flatten.py words the start of the video clash's message; a track
            # clash names the track)
            assert message.startswith(str(e.value)) and len(str(e.value)) >= 40, (cname, side)
            if cname != "unknown_image":
                assert " %d " % s.tracks["cut.long"] in str(e.value), (cname, side)
            with pytest.raises(AssertionError) as e:
                api()
            assert str(e.value) == message, (cname, side)


@pytest.mark.parametrize("name", SETS)
def test_class_api_rewrites_the_list_like_the_reference(name, recording, tmp_path):
    z, _ = recording
    s = predrules.recorded_set(name)
    gt_path = str(tmp_path / "gt.json")
    with open(gt_path, "w") as fh:
        json.dump(s.gt, fh)
    for side, make in (("lvis", lambda q: LVISResults(LVIS(gt_path), q, max_dets=s.max_dets)),
                       ("tao", lambda q: TaoResults(Tao(gt_path), q, max_dets=s.max_dets))):
        preds = copy.deepcopy(s.preds)
        make(preds)
        key = name + "_" + side
        assert [p.get("id", 0) for p in preds] == z[key + "_id"].tolist(), side
        assert [p["score"] for p in preds] == z[key + "_score"].tolist(), side
        assert [p["category_id"] for p in preds] == z[key + "_category_id"].tolist(), side
        area = np.array([p.get("area", np.nan) for p in preds], dtype=np.float64)
        assert np.array_equal(area, z[key + "_area"], equal_nan=True), side
        assert all(("segmentation" in p) == ("id" in p) for p in preds), side
