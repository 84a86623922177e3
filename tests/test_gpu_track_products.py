"""-m gpu: the host state the stages of the track analyses share on one
workspace -- which launches a sequence of stages costs (engine._valid,
engine._producing, the one share buffer), what a failed stage leaves, and
calls that alternate between thresholds at the class level.  One golden
fixture, the smaller of those test_gpu_score_curve.py runs on: the rules are
about host state, not about kernel edges."""
import numpy as np
import pytest

from tao_amodal_amd import _lib, engine
from test_gpu_identity import _tao
from test_gpu_score_curve import _same

pytestmark = pytest.mark.gpu

FIXTURE = "f4"
ALPHAS = np.arange(0.05, 0.99, 0.05) - np.finfo(float).eps
EDGES = (1, 3, 6, 11)


def _evaluated():
    ev = _tao(FIXTURE)
    ev.evaluate()
    return ev


def _count(monkeypatch, *names):
    """Wraps the bound functions `names` of the loaded library: {name: calls so far}."""
    lib, calls = _lib.load(), {}
    for name in names:
        calls[name] = 0

        def forward(*args, _name=name, _fn=getattr(lib, name)):
            calls[_name] += 1
            return _fn(*args)
        monkeypatch.setattr(lib, name, forward)
    return calls


def test_launch_counts_on_a_fresh_workspace(monkeypatch):
    ev = _evaluated()
    dp, ws = ev._run.dp, ev._run.ws
    share, assign, assign_at = ("taoamd_track_identity_share", "taoamd_track_identity_assign",
                                "taoamd_track_identity_assign_at")
    calls = _count(monkeypatch, share, assign, assign_at)
    table = np.zeros((2, dp.n_cat))
    table[1] = np.inf
    engine.stage_track_identity(dp, ws, 0.5)
    engine.stage_track_identity_at(dp, ws, 0.5, table)
    engine.stage_track_hota(dp, ws, ALPHAS, 0.5)
    engine.stage_track_clear(dp, ws, 0.5, [])
    assert calls == {share: 1, assign: 1, assign_at: 1}
    # another frame_thr: the shares are run again, into the one buffer; the identity stays
    engine.stage_track_identity_at(dp, ws, 0.75, table)
    assert calls == {share: 2, assign: 1, assign_at: 2}
    assert engine._valid(ws, "share", 0.75) and engine._valid(ws, "identity", 0.5)
    engine.stage_track_hota(dp, ws, ALPHAS, 0.5)
    assert calls == {share: 2, assign: 1, assign_at: 2}
    assert not hasattr(ws, "at_share") and not hasattr(ws, "at_frame_thr")


def test_a_failed_association_invalidates_the_followers(monkeypatch):
    ev = _evaluated()
    ev._run._followers_at("occlusions()", ev._gt_columns.ann_vis)   # the frames' visibility
    dp, ws = ev._run.dp, ev._run.ws
    engine.stage_track_association(dp, ws, 0.5, [])
    assert engine._valid(ws, "followers", 0.5)
    lib = _lib.load()
    with monkeypatch.context() as m:
        # only the host status is substituted: nothing is launched, no kernel fails
        m.setattr(lib, "taoamd_track_association", lambda *args: _lib.ERR_ARG)
        with pytest.raises(_lib.TaoAmdError, match="taoamd_track_association"):
            engine.stage_track_association(dp, ws, 0.75, [])
    assert ws.valid.get("followers") is None
    assert not engine._valid(ws, "followers", 0.5) and not engine._valid(ws, "followers", 0.75)
    ran = []
    stage = engine.stage_track_association
    monkeypatch.setattr(
        engine, "stage_track_association",
        lambda dp, ws, thr, rng: (ran.append((thr, len(rng))), stage(dp, ws, thr, rng))[1])
    engine.stage_track_occlusion(dp, ws, 0.5, 0.0, 0.1, 3, EDGES)
    assert ran == [(0.5, 0)] and engine._valid(ws, "followers", 0.5)
    engine.stage_track_occlusion(dp, ws, 0.5, 0.0, 0.1, 3, EDGES)
    assert ran == [(0.5, 0)]                                        # valid again: reused
    fresh = _evaluated()
    fresh._run._followers_at("occlusions()", fresh._gt_columns.ann_vis)
    engine.stage_track_occlusion(fresh._run.dp, fresh._run.ws, 0.5, 0.0, 0.1, 3, EDGES)
    got, want = ws.occ_counts.cpu().numpy(), fresh._run.ws.occ_counts.cpu().numpy()
    assert got.any() and np.array_equal(got, want)


def test_calls_that_alternate_between_thresholds_equal_a_fresh_evaluator():
    used = _evaluated()
    scores = np.asarray(used._run.flat.dt_score)
    t = float(np.quantile(scores, 0.5, method="lower"))
    calls = (
        ("identity", lambda ev: ev.identity()),
        ("identity at t, 0.75", lambda ev: ev.identity(score_thr=t, frame_thr=0.75)),
        ("tracking_curve", lambda ev: ev.tracking_curve()),
        ("hota", lambda ev: ev.hota(per_frame=True)),
        ("clear at 0.75", lambda ev: ev.clear(frame_thr=0.75, per_track=True, per_frame=True)),
        ("identity per track", lambda ev: ev.identity(per_track=True)))
    got = [(what, call(used)) for what, call in calls]
    for (what, result), (_, call) in zip(got, calls):
        _same(result, call(_evaluated()), what)
