"""oracle/rle.py + pyoracle.lvis_eval(iou_type="segm") (test infrastructure)
pinned to (i) the answers of the reference's own maskApi.c on seeded cases
(tests/golden/maskapi, written by tests/golden/make_golden_maskapi.py) and
(ii) the golden vectors of fixture F6 -- the reference LVISEval run with
iou_type="segm" (tests/golden/make_golden_segm.py)."""
import gzip
import json

import numpy as np
import pytest

from goldenio import path
from oracle import pyoracle, rle


def load_maskapi():
    """The reference maskApi.c's answers on seeded cases
    (tests/golden/make_golden_maskapi.py)."""
    with gzip.open(path("maskapi", "rle.json.gz"), "rt") as f:
        return json.load(f)


def test_polygon_rasterisation_and_text_form_against_reference_c():
    cases = load_maskapi()["poly"]
    assert len(cases) == 300
    for it, c in enumerate(cases):
        h, w = c["h"], c["w"]
        a = rle.fr_poly(c["xy"], h, w)
        assert a == c["rle"], it
        s = rle.to_string(a)
        assert s == c["string"]
        assert rle.fr_string(s, h, w) == a == c["fr_string"]
        assert rle.to_bbox(a) == c["bbox"]
        assert rle.area(a) == c["area"]


def test_merge_and_iou_against_reference_c():
    cases = load_maskapi()["merge"]
    assert len(cases) == 150
    for it, c in enumerate(cases):
        assert rle.merge(c["masks"], False) == c["union"], it
        assert rle.merge(c["masks"], True) == c["intersection"], it
        assert np.array_equal(rle.iou_matrix(c["dts"], c["gts"]),
                              np.asarray(c["iou"], dtype=np.float64)), it


def test_known_answers():
    full = {"h": 4, "w": 5, "counts": [0, 20]}
    half = {"h": 4, "w": 5, "counts": [0, 8, 12]}          # the two left columns
    assert rle.iou_pair(full, half) == 8 / 20
    assert rle.iou_pair(half, half) == 1.0
    right = {"h": 4, "w": 5, "counts": [12, 8]}
    assert rle.iou_pair(half, right) == 0.0
    assert rle.to_bbox(right) == [3.0, 0.0, 2.0, 4.0]
    assert rle.merge([half, right])["counts"] == [0, 8, 4, 8]
    assert rle.merge([half, full], intersect=True)["counts"] == [0, 8, 12]
    # a 3 x 2 box drawn as a polygon on a 6 x 8 frame
    box = rle.fr_bbox([2, 1, 3, 2], 6, 8)
    assert rle.area(box) == 6 and rle.to_bbox(box) == [2.0, 1.0, 3.0, 2.0]


def load_segm():
    with gzip.open(path("f6", "lvis_segm.json.gz")) as f:
        g = json.load(f)
    z = np.load(path("f6", "lvis_segm.npz"))
    return g, z


@pytest.mark.parametrize("which", ["pred", "pred_rle"])
def test_lvis_oracle_segm_matches_reference(which):
    golden, z = load_segm()
    w = golden[which]
    gt = json.load(open(path("f6", "gt.json")))
    pred = json.load(open(path("f6", which + ".json")))
    got = pyoracle.lvis_eval(gt, pred, iou_type="segm")
    # every mask the evaluator compared, as compressed text
    assert {str(k): v for k, v in got["gt_rle"].items()} == w["gt_rle"]
    assert {str(k): v for k, v in got["dt_rle"].items()} == w["dt_rle"]
    assert {str(k): v for k, v in got["dt_area"].items()} == w["dt_area"]
    assert {str(k): v for k, v in got["dt_bbox"].items()} == w["dt_bbox"]
    want_cells = {tuple(c["key"]): np.asarray(c["ious"], dtype=float) for c in w["cells"]}
    have = {k: c for k, c in got["cells"].items() if np.asarray(c["ious"]).size}
    assert set(have) == set(want_cells)
    for k, c in have.items():
        assert np.array_equal(np.asarray(c["ious"]), want_cells[k].reshape(np.asarray(c["ious"]).shape)), k
    evals = {tuple(e["key"]): e for e in w["evals"]}
    n = 0
    for (im, c), cell in got["cells"].items():
        for a, e in enumerate(cell["ranges"]):
            r = evals[im, c, a]
            assert [int(x) for x in e["dt_ids"]] == r["dt_ids"]
            assert [int(x) for x in e["gt_ids"]] == r["gt_ids"]
            for key in ("dt_matches", "dt_ignore", "gt_ignore"):
                mine = np.asarray(e[key]).astype(int)
                assert np.array_equal(mine, np.asarray(r[key]).reshape(mine.shape)), (im, c, a, key)
            n += 1
    assert n == len(evals)
    assert np.array_equal(got["precision"], z[which + "_precision"])
    assert np.array_equal(got["recall"], z[which + "_recall"])
    assert [[k, float(v)] for k, v in got["results"].items()] == w["results"]
