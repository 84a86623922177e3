"""What is made from the input columns and reused -- device copies
(flatten_dev.device_copy), the top-max_dets cut, prepared ground-truth halves --
follows columns.array_key: a rebound column and an in-place edit that touches a
sampled element are seen, any other edit after flatten_dev.forget_columns.
Torch's CPU device stands in for the GPU."""
import gc

import numpy as np
import pytest

from tao_amodal_amd import engine, flatten, flatten_dev
from tao_amodal_amd.synth import synth


def _problem(gt, dt, kind):
    f = flatten.flatten_lvis(gt, dt) if kind == "lvis" else flatten.flatten_tao(gt, dt)
    return f, engine.DeviceProblem(f, "cpu")


def _inputs():
    gt, dt = synth(seed=31, V=3, F=30, C=11, dets_per_frame=30, n_present=4)
    assert len(dt) > 2048                           # (fingerprint skips elements)
    dt.track_id, _ = flatten.make_track_ids_unique(dt)
    return gt, dt


def _unsampled(a, among=None):
    """The first flat index of `a` (of `among`) that columns.fingerprint does
    not read."""
    step = max(1, a.size // 1024)
    among = range(a.size) if among is None else among
    return next(int(i) for i in among if i % step and i != a.size - 1)


@pytest.mark.parametrize("kind, name", [("lvis", "dt_box"), ("tao", "dt_frame_box")])
@pytest.mark.parametrize("order", ["C", "F"])
def test_host_build_sees_an_in_place_box_edit(kind, name, order):
    gt, dt = _inputs()
    # ("F": a table the upload has to copy even where a CPU tensor could
    # share the array's memory)
    dt.bbox = np.asarray(dt.bbox, order=order)
    f, dp = _problem(gt, dt, kind)
    assert np.array_equal(dp.t[name].numpy(), np.asarray(f[name]))
    dt.bbox[:, 0] += 0.5                          # every row: the samples too
    f, dp = _problem(gt, dt, kind)
    assert np.array_equal(dp.t[name].numpy(), np.asarray(f[name]))


def test_an_unsampled_edit_is_seen_after_forget_columns():
    gt, dt = _inputs()
    i = _unsampled(dt.score)
    before = flatten_dev.raw_columns(dt, "cpu")["score"][i].item()
    dt.score[i] = 0.125
    assert flatten_dev.raw_columns(dt, "cpu")["score"][i].item() == before
    flatten_dev.forget_columns(dt)
    assert flatten_dev.raw_columns(dt, "cpu")["score"][i].item() == 0.125
    # the boxes of the host-built tables as well
    f, dp = _problem(gt, dt, "lvis")
    j = _unsampled(dt.bbox, 4 * np.asarray(f.dt_row, np.int64) + 1)
    row = int(np.flatnonzero(f.dt_row == j // 4)[0])
    dt.bbox.reshape(-1)[j] += 1.0
    f, dp = _problem(gt, dt, "lvis")
    assert dp.t["dt_box"][row, j % 4].item() != f.dt_box[row][j % 4]
    flatten_dev.forget_columns(dt)
    f, dp = _problem(gt, dt, "lvis")
    assert np.array_equal(dp.t["dt_box"].numpy(), np.asarray(f.dt_box))


def test_a_rebound_column_is_uploaded_again_and_the_others_are_not():
    _, dt = _inputs()
    a = flatten_dev.raw_columns(dt, "cpu")
    dt.score = dt.score * 0.5
    b = flatten_dev.raw_columns(dt, "cpu")
    assert b["score"] is not a["score"]
    assert np.array_equal(b["score"].numpy(), dt.score)
    for name in ("image_id", "category_id", "bbox", "video_id"):
        assert b[name] is a[name], name


def test_a_cache_entry_goes_away_with_its_array():
    a = np.arange(5000, dtype=np.float64)
    t = flatten_dev.device_copy(a, "cpu")
    assert flatten_dev.device_copy(a, "cpu") is t
    assert t.data_ptr() != a.ctypes.data            # a copy, also on the CPU
    k = id(a)
    assert k in flatten_dev._COPIES
    del a
    gc.collect()
    assert k not in flatten_dev._COPIES
    assert float(t[4999]) == 4999.0                 # (the caller's tensor stays)
    _, dt = _inputs()
    ids = [id(getattr(dt, n)) for n in ("image_id", "category_id", "score", "bbox")]
    flatten_dev.raw_columns(dt, "cpu")
    assert all(k in flatten_dev._COPIES for k in ids)
    del dt
    gc.collect()
    assert not any(k in flatten_dev._COPIES for k in ids)


def test_limit_dets_per_image_sees_an_in_place_score_edit():
    _, dt = _inputs()
    keep = flatten.limit_dets_per_image(dt, 10)
    assert flatten.limit_dets_per_image(dt, 10) is keep
    dt.score *= -1.0
    got = flatten.limit_dets_per_image(dt, 10)
    want = flatten.limit_dets_per_image(dt.take(np.arange(len(dt))), 10)
    assert np.array_equal(got, want) and not np.array_equal(got, keep)
    # an unsampled edit: after forget_columns
    i = _unsampled(dt.score)
    dt.score[i] = 10.0
    assert flatten.limit_dets_per_image(dt, 10) is got
    flatten_dev.forget_columns(dt)
    want = flatten.limit_dets_per_image(dt.take(np.arange(len(dt))), 10)
    assert not np.array_equal(want, got)
    assert np.array_equal(flatten.limit_dets_per_image(dt, 10), want)


def test_forget_columns_drops_a_prepared_ground_truth_half():
    gt, dt = _inputs()
    flatten_dev.prepare_gt(gt, wait=False)
    assert "_prepared_gt" in vars(gt)
    _problem(gt, dt, "tao")                         # (uploads gt.ann_bbox)
    assert id(gt.ann_bbox) in flatten_dev._COPIES
    flatten_dev.forget_columns(gt)
    assert "_prepared_gt" not in vars(gt) and id(gt.ann_bbox) not in flatten_dev._COPIES
