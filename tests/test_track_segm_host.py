"""TaoEval(iou_type="segm"), the host side: Tao.ann_to_rle, mask-only
predictions in TaoResults, the frames' annotation rows of the track tables,
the per-frame masks, the restatement of the metric (tests/track_segm_ref.py)
on hand cases, and what stays out of scope.  No GPU needed."""
import copy
import json
import types

import numpy as np
import pytest

import track_segm_ref as ref
from goldenio import path
from oracle import rle
from tao_amodal_amd import flatten
from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval, TaoResults


def _load(name):
    with open(path("f6", name)) as f:
        return json.load(f)


def _text(r):
    c = r["counts"]
    return c.decode() if isinstance(c, bytes) else c


def test_tao_ann_to_rle_equals_the_oracle_on_every_f6_annotation():
    """one polygon, several polygons, uncompressed and compressed RLE"""
    gt = Tao(path("f6", "gt.json"))
    kinds = set()
    for a in gt.dataset["annotations"]:
        im = gt.imgs[a["image_id"]]
        s = a["segmentation"]
        kinds.add("poly%d" % min(len(s), 2) if isinstance(s, list)
                  else type(s["counts"]).__name__)
        got = gt.ann_to_rle(a)
        want = rle.ann_to_rle(s, im["height"], im["width"])
        assert _text(got) == rle.to_string(want), a["id"]
        assert list(got["size"]) == [want["h"], want["w"]]
    assert kinds == {"poly1", "poly2", "list", "str"}
    with pytest.raises(KeyError):
        gt.ann_to_rle({k: v for k, v in gt.dataset["annotations"][0].items()
                       if k != "segmentation"})


@pytest.mark.parametrize("as_list", [False, True])
def test_mask_only_predictions_build_tracks_with_mask_area_and_box(as_list):
    gt = Tao(path("f6", "gt.json"))
    preds = _load("pred_rle.json")
    assert all("bbox" not in p for p in preds)
    res = TaoResults(gt, copy.deepcopy(preds) if as_list else path("f6", "pred_rle.json"))
    masks = [rle.ann_to_rle(p["segmentation"], 0, 0) for p in preds]
    dt = res.columns_dt
    assert np.array_equal(dt.area, [rle.area(m) for m in masks])
    assert np.array_equal(dt.bbox, np.array([rle.to_bbox(m) for m in masks], float))
    f = flatten.flatten_tao(gt.columns, dt)
    rows = np.asarray(f.dt_frame_ann)
    assert len(rows) and np.array_equal(np.asarray(f.dt_frame_box), dt.bbox[rows])
    # a track's area is the mean of its masks' areas
    off = np.asarray(f.dt_frame_off)
    for t in range(len(off) - 1):
        if off[t + 1] - off[t] == 1:
            assert f.dt_area[t] == rle.area(masks[rows[off[t]]])


def test_frame_masks_use_the_segmentation_or_the_box_polygon():
    """f6/pred.json: a third of the predictions bring a polygon, the others
    only a box -- their frames take the box's polygon."""
    gt = Tao(path("f6", "gt.json"))
    preds = _load("pred.json")
    ev = TaoEval(gt, path("f6", "pred.json"), iou_type="segm")
    f = flatten.flatten_tao(gt.columns, ev.tao_dt.columns_dt)
    got = ev._masks(f)
    want_dt, want_gt = ref.frame_masks(f, gt.dataset, preds)
    rows = np.asarray(f.dt_frame_ann).tolist()
    assert any("segmentation" in preds[r] for r in rows)
    assert any("segmentation" not in preds[r] for r in rows)
    for side, want in (("dt", want_dt), ("gt", want_gt)):
        m = got[side]
        assert len(m) == len(want)
        for k, w in enumerate(want):
            assert m.mask(k) == w, (side, k)


def _with_duplicates():
    """F6 with a second annotation / prediction on an image its track already
    covers (another box): the frame keeps one of the two."""
    g, p = _load("gt.json"), _load("pred.json")
    a = copy.deepcopy(g["annotations"][0])
    a["id"] = max(x["id"] for x in g["annotations"]) + 1
    a["bbox"] = [a["bbox"][0] + 1.5, a["bbox"][1], a["bbox"][2], a["bbox"][3] - 1]
    g["annotations"].append(a)
    d = copy.deepcopy(p[0])
    d["bbox"] = [d["bbox"][0] + 2.0, d["bbox"][1] + 1.0, d["bbox"][2], d["bbox"][3]]
    p.append(d)
    return g, p, len(g["annotations"]) - 1, len(p) - 1


@pytest.mark.parametrize("use_cats", [True, False])
def test_frame_ann_names_the_annotation_of_every_frame_box(use_cats):
    g, p, dup_gt, dup_dt = _with_duplicates()
    gt = Tao(g)
    dt = TaoResults(gt, p).columns_dt
    f = flatten.flatten_tao(gt.columns, dt, use_cats=use_cats)
    for side, boxes, dup, first in (("dt", dt.bbox, dup_dt, 0),
                                    ("gt", gt.columns.ann_bbox, dup_gt, 0)):
        rows = np.asarray(f[side + "_frame_ann"])
        assert rows.dtype == np.int64 and len(rows) == len(f[side + "_frame_pos"])
        assert np.array_equal(np.asarray(f[side + "_frame_box"]), boxes[rows]), side
        # one of the two annotations of the doubled frame, not both
        assert (np.isin([dup, first], rows)).sum() == 1, side


def test_restatement_hand_cases():
    sq = {"h": 4, "w": 4, "counts": [5, 2, 2, 2, 5]}            # 2 x 2 block
    other = {"h": 4, "w": 4, "counts": [0, 3, 13]}              # 3 pixels
    for mode in ("3d_iou", "avg_iou", "imagenetvid"):
        # identical tracks
        t = {0: sq, 3: other, 7: sq}
        assert ref.track_iou(t, dict(t), mode) == 1.0
        # disjoint frame sets
        assert ref.track_iou({0: sq, 1: sq}, {2: sq, 3: sq}, mode) == 0.0
    # mismatched frame size: that frame contributes 0 / 0
    small = {"h": 2, "w": 2, "counts": [0, 4]}
    assert ref.frame_terms(sq, small) == (0, 0)
    assert ref.track_iou({0: sq, 1: sq}, {0: sq, 1: small}, "3d_iou") == 4 / 4
    assert ref.track_iou({0: sq, 1: sq}, {0: sq, 1: small}, "avg_iou") == 1 / 2
    assert ref.track_iou({0: sq, 1: sq}, {0: sq, 1: small}, "imagenetvid") == 1 / 2
    # both masks empty: u = 0
    empty = {"h": 4, "w": 4, "counts": [16]}
    assert ref.frame_terms(empty, empty) == (0, 0)
    assert ref.track_iou({0: empty}, {0: empty}, "3d_iou") == 0.0
    assert ref.track_iou({0: empty}, {0: empty}, "avg_iou") == 0.0
    # partial overlap, a frame only one side has
    assert ref.frame_terms(sq, other) == (0, 7)
    half = {"h": 4, "w": 4, "counts": [5, 2, 9]}                # 2 of sq's 4
    assert ref.frame_terms(sq, half) == (2, 4)
    assert ref.track_iou({0: sq, 1: half}, {0: half}, "3d_iou") == 2 / (4 + 2)
    assert ref.track_iou({0: sq, 1: half}, {0: half}, "avg_iou") == (2 / 4) / 2
    assert ref.track_iou({0: sq, 1: sq}, {0: half, 1: sq}, "imagenetvid") == 1 / 2


def test_box_polygons_of_integer_boxes_are_the_rectangles():
    """What the rectangle-equivalence test on the GPU rests on: an integer box
    inside the frame rasterises to w * h pixels, and two such masks intersect
    in exactly the boxes' intersection."""
    rng = np.random.default_rng(3)
    H, W = 40, 56
    for _ in range(200):
        boxes = []
        for _ in range(2):
            x, y = int(rng.integers(0, W - 1)), int(rng.integers(0, H - 1))
            w, h = int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))
            boxes.append([x, y, w, h])
        m = [rle.ann_to_rle(ref.box_polygon(b), H, W) for b in boxes]
        assert [rle.area(x) for x in m] == [b[2] * b[3] for b in boxes]
        (ax, ay, aw, ah), (bx, by, bw, bh) = boxes
        iw = max(0, min(ax + aw, bx + bw) - max(ax, bx))
        ih = max(0, min(ay + ah, by + bh) - max(ay, by))
        assert ref.frame_terms(m[0], m[1]) == (iw * ih, aw * ah + bw * bh - iw * ih)


def test_segm_out_of_scope_raises():
    gt = Tao(path("f6", "gt.json"))
    ev = TaoEval(gt, path("f6", "pred.json"), iou_type="segm")
    ev.params.vid_ids = ev.params.vid_ids[:1]
    with pytest.raises(NotImplementedError, match="vid_ids"):
        ev.evaluate()
    ev = TaoEval(gt, path("f6", "pred.json"), iou_type="segm",
                 dist=types.SimpleNamespace(device="cpu"))
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        ev.evaluate()
