"""What the image and the track level share of the on-request error analyses,
without a GPU and without the library: the two text tables against lines
recorded from the classes' own formatters before they were merged, the
threshold validation behind the cache key, and the engine stages' refusal of a
problem of the other level."""
import types

import numpy as np
import pytest

from tao_amodal_amd import _lib, engine
from tao_amodal_amd.evaluation import _core
from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
from tao_amodal_amd.evaluation.tao_amodal import TaoEval


def _types_table(rng_lbl):
    """Two ranges, two categories, every cell distinct."""
    dt = np.arange(1, 29, dtype=np.int64).reshape(2, 2, 7) * 3
    gt = np.arange(1, 13, dtype=np.int64).reshape(2, 2, 3) * 1000 + 7
    return {"types": list(_lib.ERROR_TYPES), "dt_counts": dt, "gt_counts": gt,
            "rng_lbl": rng_lbl}


def _impact_table(rng_lbl):
    ap = (np.arange(1, 19, dtype=np.float64) ** 2).reshape(9, 2) / 400
    return {"fixes": list(_lib.ERROR_FIXES), "precision": None, "ap": ap,
            "dap": ap[1:] - ap[0], "rng_lbl": rng_lbl}


def _stubbed(cls, rng_lbl):
    """An evaluator whose tables are the hand-written ones; ONE label for two
    ranges: the second line goes by its index."""
    ev = cls.__new__(cls)
    ev.error_types = lambda iou_thr=0.5, bg_thr=0.1, per_detection=False: _types_table(rng_lbl)
    ev.error_impact = lambda iou_thr=0.5, bg_thr=0.1: _impact_table(rng_lbl)
    return ev


TYPE_COLS = ("         TP    IGNORED        DUP        LOC        CLS       BOTH        BKG"
             "         GT     missed missed_loc")
TYPE_ROWS = ("         27         33         39         45         51         57         63"
             "       5014       7014       9014",
             "        111        117        123        129        135        141        147"
             "      17014      19014      21014")
IMPACT_COLS = "       AP     dCLS     dLOC    dBOTH     dDUP     dBKG    dMISS      dFP      dFN"
IMPACT_ROWS = ("   0.0025   0.0200   0.0600   0.1200   0.2000   0.3000   0.4200   0.5600   0.7200",
               "   0.0100   0.0300   0.0800   0.1500   0.2400   0.3500   0.4800   0.6300   0.8000")


def test_image_level_lines_are_the_recorded_ones():
    ev = _stubbed(LVISEval, ["highly-occluded"])        # (wider than the 10 columns' minimum)
    assert ev.error_lines(0.75, 0.25) == [
        " error types @[ IoU=0.75 | bg=0.25 ]",
        "                " + TYPE_COLS,
        " highly-occluded" + TYPE_ROWS[0],
        " 1              " + TYPE_ROWS[1]]
    assert ev.impact_lines(0.75, 0.25) == [
        " error impact @[ IoU=0.75 | bg=0.25 ]",
        "                " + IMPACT_COLS,
        " highly-occluded" + IMPACT_ROWS[0],
        " 1              " + IMPACT_ROWS[1]]


def test_track_level_lines_are_the_recorded_ones():
    ev = _stubbed(TaoEval, [("all", "all")])
    assert ev.error_lines(0.75, 0.25) == [
        " track error types @[ IoU=0.75 | bg=0.25 ]",
        "           " + TYPE_COLS,
        " all/all   " + TYPE_ROWS[0],
        " 1         " + TYPE_ROWS[1]]
    assert ev.impact_lines(0.75, 0.25) == [
        " track error impact @[ IoU=0.75 | bg=0.25 ]",
        "           " + IMPACT_COLS,
        " all/all   " + IMPACT_ROWS[0],
        " 1         " + IMPACT_ROWS[1]]


def test_error_key_finds_the_threshold_and_bounds_bg_thr():
    thrs = np.linspace(0.5, 0.95, 10)
    assert _core.error_key(thrs, 0.5, 0.1) == (0, 0.1)
    assert _core.error_key(thrs, thrs[5], 0) == (5, 0.0)
    assert _core.error_key(list(thrs), thrs[9], 0.5) == (9, 0.5)
    key = _core.error_key(thrs, 0.5, np.float32(0.25))
    assert key == (0, 0.25) and type(key[0]) is int and type(key[1]) is float
    # tf = min(iou_thr, 1 - 1e-10): a threshold of 1 admits what lies below the clamp
    assert _core.error_key([1.0], 1.0, 1 - 2e-10) == (0, 1 - 2e-10)
    for iou_thr in (0.55000001, 0.4, 1.0):
        with pytest.raises(ValueError, match="iou_thr: .* is not one of params.iou_thrs"):
            _core.error_key(thrs, iou_thr, 0.1)
    for iou_thr, bg_thr in ((0.5, 0.5), (0.5, 0.75), (0.5, -0.1), (0.5, float("nan")),
                            (thrs[5], thrs[5])):
        with pytest.raises(ValueError, match=r"bg_thr: .* is not in \[0, "):
            _core.error_key(thrs, iou_thr, bg_thr)
    with pytest.raises(ValueError, match=r"bg_thr: .* is not in \[0, "):
        _core.error_key([1.0], 1.0, 1 - 1e-10)
    # the threshold is looked up first
    with pytest.raises(ValueError, match="iou_thr"):
        _core.error_key(thrs, 0.4, -1)


@pytest.mark.parametrize("stage, kind, words", [
    ("stage_error_types", "tao", "the error breakdown is the image level's, on boxes"),
    ("stage_error_impact", "tao", "the error breakdown is the image level's, on boxes"),
    ("stage_track_error_types", "lvis",
     "the track-level error breakdown is the track level's, on boxes"),
    ("stage_track_error_impact", "lvis",
     "the track-level error breakdown is the track level's, on boxes")])
def test_a_stage_refuses_the_other_level_ahead_of_the_library(monkeypatch, stage, kind, words):
    def no_library():
        raise AssertionError("the refusal comes before the library is loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    dp = types.SimpleNamespace(kind=kind, mask_iou=False, iou_mode=0,
                               cell_unit_host=np.zeros(1, np.int64))
    with pytest.raises(_lib.TaoAmdError) as err:
        getattr(engine, stage)(dp, None, 0, 0.1)
    assert str(err.value) == words
