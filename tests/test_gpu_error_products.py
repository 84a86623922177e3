"""-m gpu: the host state of the error breakdown, its impact and its confusion on
one workspace, at both levels -- which launches a sequence of the stages costs,
what a failed match leaves (the product "match indices"), and the documented
give-backs of their buffers.  One golden fixture a level: the rules are about
host state, not about kernel edges."""
import numpy as np
import pytest

from tao_amodal_amd import _lib, engine
from test_gpu_error_types import _lvis
from test_gpu_identity import _tao
from test_gpu_track_products import _count

pytestmark = pytest.mark.gpu

SLOT, BG_THR = 0, 0.1
# level: (evaluator, breakdown stage, impact stage, breakdown entry point, impact entry point)
LEVELS = {
    "image": (lambda: _lvis("f1", None, pred="pred.json"), "stage_error_types",
              "stage_error_impact", "taoamd_error_types", "taoamd_error_impact"),
    "track": (lambda: _tao("f4"), "stage_track_error_types", "stage_track_error_impact",
              "taoamd_track_error_types", "taoamd_track_error_impact")}
IMPACT = ("err_dt_counts", "err_gt_counts", "err_dt_type", "err_link_same", "err_link_other",
          "err_held", "imp_precision", "imp_num_gt")


def _evaluated(level):
    ev = LEVELS[level][0]()
    ev.evaluate()
    return ev._run.dp, ev._run.ws


def _tables(ws, names):
    out = {n: getattr(ws, n).cpu().numpy() for n in names}
    if "conf_off" in out:
        out["conf_gt_cat"] = ws.conf_gt_cat[:ws.conf_n].cpu().numpy()
        out["conf_counts"] = ws.conf_counts[:ws.conf_n].cpu().numpy()
    return out


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_launch_counts_on_a_fresh_workspace(level, monkeypatch):
    _, types, impact, types_entry, impact_entry = LEVELS[level]
    dp, ws = _evaluated(level)
    calls = _count(monkeypatch, "taoamd_match", types_entry, types_entry + "_links", impact_entry,
                   "taoamd_confusion_count", "taoamd_confusion_fill")
    getattr(engine, types)(dp, ws, SLOT, BG_THR)
    getattr(engine, types)(dp, ws, SLOT, BG_THR, per_detection=True)
    getattr(engine, impact)(dp, ws, SLOT, BG_THR)
    engine.stage_confusion(dp, ws, SLOT, BG_THR)
    assert calls == {"taoamd_match": 1, types_entry: 2, types_entry + "_links": 2,
                     impact_entry: 1, "taoamd_confusion_count": 1, "taoamd_confusion_fill": 1}
    assert engine._valid(ws, "match indices", ())


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_a_failed_match_invalidates_the_indices(level, monkeypatch):
    types = getattr(engine, LEVELS[level][1])
    dp, ws = _evaluated(level)
    lib = _lib.load()
    with monkeypatch.context() as m:
        # only the host status is substituted: nothing is launched, no kernel fails
        m.setattr(lib, "taoamd_match", lambda *args: _lib.ERR_ARG)
        with pytest.raises(_lib.TaoAmdError, match="taoamd_match"):
            types(dp, ws, SLOT, BG_THR)
    assert ws.err_match_gt is not None and "match indices" not in ws.valid
    calls = _count(monkeypatch, "taoamd_match")
    types(dp, ws, SLOT, BG_THR)
    assert calls == {"taoamd_match": 1} and engine._valid(ws, "match indices", ())
    types(dp, ws, SLOT, BG_THR)
    assert calls == {"taoamd_match": 1}                             # valid again: reused
    fresh_dp, fresh_ws = _evaluated(level)
    types(fresh_dp, fresh_ws, SLOT, BG_THR)
    got, want = (_tables(w, ("err_dt_counts", "err_gt_counts")) for w in (ws, fresh_ws))
    assert got["err_dt_counts"].any()
    for name in got:
        assert np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_buffers_given_back_are_allocated_again(level):
    impact = getattr(engine, LEVELS[level][2])
    dp, ws = _evaluated(level)
    impact(dp, ws, SLOT, BG_THR)
    first = _tables(ws, IMPACT)
    engine.stage_confusion(dp, ws, SLOT, BG_THR)
    first.update(_tables(ws, ("conf_off",)))
    assert first["imp_num_gt"].any() and ws.conf_n > 0
    # the three give-backs of the docstrings
    ws.err_link_same = ws.err_link_other = ws.imp_ws = None
    ws.err_match_gt = None
    ws.conf_ws = ws.conf_off = ws.conf_gt_cat = ws.conf_counts = None
    impact(dp, ws, SLOT, BG_THR)
    again = _tables(ws, IMPACT)
    engine.stage_confusion(dp, ws, SLOT, BG_THR)
    again.update(_tables(ws, ("conf_off",)))
    given_back = ("err_link_same", "err_link_other", "imp_ws", "err_match_gt", "conf_ws",
                  "conf_off", "conf_gt_cat", "conf_counts")
    assert all(getattr(ws, n) is not None for n in given_back)
    assert sorted(again) == sorted(first)
    for name in first:
        assert np.array_equal(first[name], again[name]), name
