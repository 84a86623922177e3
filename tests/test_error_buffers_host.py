"""No GPU: the host rules of the four older on-request analyses (stage_scores,
the error breakdown, its impact, its confusion) on a bare workspace with CPU
tensors -- their declaration, their buffers under engine._stage_buffers /
engine._buffer with the documented give-backs, and the product "match indices"
of ws.err_match_gt."""
import types

import pytest
import torch

from tao_amodal_amd import engine

CPU = torch.device("cpu")
u8, i32, i64, f64 = torch.uint8, torch.int32, torch.int64, torch.float64

# every ws attribute the four stages assign
ASSIGNED = (
    "score_ws", "score_bytes", "scores", "score_order",
    "err_ws", "err_bytes", "err_match_gt", "err_dt_counts", "err_gt_counts", "err_dt_type",
    "err_link_same", "err_link_other", "err_held",
    "imp_ws", "imp_bytes", "imp_precision", "imp_num_gt", "imp_order",
    "conf_ws", "conf_bytes", "conf_off", "conf_gt_cat", "conf_counts", "conf_n")

# the documented give-backs (error_match_gt, stage_error_impact, stage_confusion)
GIVE_BACKS = (("err_link_same", "err_link_other", "imp_ws"), ("err_match_gt",),
              ("conf_ws", "conf_off", "conf_gt_cat", "conf_counts"))

SIZES = [(0, 0, 1, 1), (3, 2, 2, 2)]
KINDS = ["lvis", "tao"]


class StubLib:
    """The *_workspace functions of the library, with fixed byte counts."""
    taoamd_score_at_recall_workspace = staticmethod(lambda n_dt, n_cat, n_rng: 40)
    taoamd_error_types_workspace = staticmethod(lambda n_dt, n_gt, n_rng: 1000)
    taoamd_track_error_types_workspace = staticmethod(lambda n_dt, n_gt, n_rng: 3000)
    taoamd_error_impact_workspace = staticmethod(lambda n_dt, n_gt, n_cat, n_rng: 100)
    taoamd_track_error_impact_workspace = staticmethod(lambda n_dt, n_gt, n_cat, n_rng: 700)
    taoamd_confusion_workspace = staticmethod(lambda n_dt, n_gt, n_cat, n_rng: 0)


def _problem(kind, n_dt, n_gt, n_cat, n_rng):
    return types.SimpleNamespace(kind=kind, n_dt=n_dt, n_gt=n_gt, n_cat=n_cat, n_rng=n_rng,
                                 device=CPU)


@pytest.fixture
def ws():
    w = object.__new__(engine.Workspace)
    w.declare_products()
    w.match_gt, w.cell_order = None, False
    return w


def _request(dp, ws, per_detection=False, links=False):
    """What a breakdown, an impact and a confusion of `dp` ask for, the last with 5 entries."""
    lib = StubLib()
    engine._error_buffers(dp, ws, lib, per_detection, links)
    if links:
        engine._impact_buffers(dp, ws, lib, "taoamd_error_impact" if dp.kind == "lvis"
                               else "taoamd_track_error_impact")
        engine._confusion_buffers(dp, ws, lib)
        engine._confusion_entries(dp, ws, 5)


def _storage(ws):
    return {n: getattr(ws, n).data_ptr() for n in ASSIGNED
            if isinstance(getattr(ws, n), torch.Tensor)}


def _is(t, shape, dtype):
    return tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()


def test_every_product_is_declared_once(ws):
    names = engine.Workspace.ANALYSIS_PRODUCTS + engine.Workspace.TRACK_PRODUCTS
    assert len(set(names)) == len(names)
    assert set(ASSIGNED) <= set(names)
    assert all(getattr(ws, n) is None for n in names) and ws.valid == {}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_dt,n_gt,n_cat,n_rng", SIZES)
def test_breakdown_buffers(ws, kind, n_dt, n_gt, n_cat, n_rng):
    dp = _problem(kind, n_dt, n_gt, n_cat, n_rng)
    _request(dp, ws)
    nbytes = 1000 if kind == "lvis" else 3000
    assert ws.err_bytes == nbytes and _is(ws.err_ws, (nbytes,), u8)
    assert _is(ws.err_dt_counts, (n_rng, n_cat, 7), i64)
    assert _is(ws.err_gt_counts, (n_rng, n_cat, 3), i64)
    # the optional tables: only when first asked for
    optional = ("err_dt_type", "err_link_same", "err_link_other", "err_held")
    assert all(getattr(ws, n) is None for n in optional + ("imp_ws", "conf_ws", "err_match_gt"))
    first = _storage(ws)
    _request(dp, ws)
    assert _storage(ws) == first
    _request(dp, ws, per_detection=True)
    assert _is(ws.err_dt_type, (max(n_dt, 1), n_rng), u8)
    assert all(getattr(ws, n) is None for n in optional[1:])
    _request(dp, ws, per_detection=True, links=True)
    assert _is(ws.err_link_same, (max(n_dt, 1), n_rng), i32)
    assert _is(ws.err_link_other, (max(n_dt, 1), n_rng), i32)
    assert _is(ws.err_held, (n_rng, max(n_gt, 1)), u8)
    nbytes = 100 if kind == "lvis" else 700
    assert ws.imp_bytes == nbytes and _is(ws.imp_ws, (max(nbytes, 256),), u8)
    assert _is(ws.imp_precision, (9, 101, n_cat, n_rng), f64)
    assert _is(ws.imp_num_gt, (9, n_cat, n_rng), i32)
    assert ws.conf_bytes == 0 and _is(ws.conf_ws, (256,), u8)
    assert _is(ws.conf_off, (n_rng * n_cat + 1,), i64)
    assert ws.conf_n == 5 and _is(ws.conf_gt_cat, (5,), i32) and _is(ws.conf_counts, (5, 4), i32)
    # once there, they stay: with a request that does not name them, and with a second
    # identical one
    held = _storage(ws)
    assert {n: p for n, p in held.items() if n in first} == first
    _request(dp, ws)
    _request(dp, ws, per_detection=True, links=True)
    _request(dp, ws, per_detection=True, links=True)
    assert _storage(ws) == held


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("names", GIVE_BACKS)
def test_give_back(ws, kind, names):
    dp = _problem(kind, 3, 2, 2, 2)
    _request(dp, ws, per_detection=True, links=True)
    _request(dp, ws, per_detection=True, links=True)            # (a steady state)
    engine.error_match_gt(dp, ws)
    held = {n: getattr(ws, n) for n in ASSIGNED}
    for n in names:
        setattr(ws, n, None)
    _request(dp, ws, per_detection=True, links=True)
    engine.error_match_gt(dp, ws)
    for n in ASSIGNED:
        now = getattr(ws, n)
        if n in names:
            # allocated again, as it was (the old one is alive in `held`: another storage)
            assert now is not None and now is not held[n]
            assert _is(now, tuple(held[n].shape), held[n].dtype)
        else:
            assert now is held[n], n


def test_confusion_entries(ws):
    dp = _problem("lvis", 3, 2, 2, 2)
    engine._confusion_entries(dp, ws, 0)
    assert ws.conf_n == 0 and _is(ws.conf_gt_cat, (1,), i32) and _is(ws.conf_counts, (1, 4), i32)
    engine._confusion_entries(dp, ws, 5)
    assert ws.conf_n == 5 and _is(ws.conf_gt_cat, (5,), i32) and _is(ws.conf_counts, (5, 4), i32)
    five = ws.conf_gt_cat, ws.conf_counts
    engine._confusion_entries(dp, ws, 3)
    assert ws.conf_n == 3 and ws.conf_gt_cat is five[0] and ws.conf_counts is five[1]
    engine._confusion_entries(dp, ws, 9)
    assert ws.conf_n == 9 and _is(ws.conf_gt_cat, (9,), i32) and _is(ws.conf_counts, (9, 4), i32)
    assert ws.conf_gt_cat is not five[0] and ws.conf_counts is not five[1]


def _record(monkeypatch, name="stage_match", fail=()):
    """engine.<name> as a recorder of the match_gt it is handed; raises on the calls
    whose number is in `fail`."""
    calls = []

    def recorder(dp, ws, *args, **kwargs):
        calls.append(kwargs["match_gt"] if "match_gt" in kwargs else args[-1])
        if len(calls) in fail:
            raise RuntimeError("the match failed")
    monkeypatch.setattr(engine, name, recorder)
    return calls


def test_match_indices_are_a_product(ws, monkeypatch):
    dp = _problem("lvis", 3, 2, 2, 2)
    calls = _record(monkeypatch)
    assert not engine._valid(ws, "match indices", ())
    table = engine._error_match_gt(dp, ws)
    assert table is ws.err_match_gt and _is(table, (3, 20), i32)
    assert len(calls) == 1 and calls[0] is table and engine._valid(ws, "match indices", ())
    assert engine._error_match_gt(dp, ws) is table and len(calls) == 1
    # given back: a new table, and the match again
    ws.err_match_gt = None
    again = engine._error_match_gt(dp, ws)
    assert again is not None and again is not table and len(calls) == 2 and calls[1] is again


def test_allocation_alone_validates_nothing(ws, monkeypatch):
    dp = _problem("tao", 3, 2, 2, 2)
    calls = _record(monkeypatch)
    table = engine.error_match_gt(dp, ws)
    assert _is(table, (3, 20), i32) and engine.error_match_gt(dp, ws) is table
    assert ws.valid == {}
    assert engine._error_match_gt(dp, ws) is table and len(calls) == 1
    # nor does the allocation after a give-back
    ws.err_match_gt = None
    table = engine.error_match_gt(dp, ws)
    assert not engine._valid(ws, "match indices", ())
    assert engine._error_match_gt(dp, ws) is table and len(calls) == 2


def test_a_failed_match_leaves_the_indices_invalid(ws, monkeypatch):
    dp = _problem("lvis", 3, 2, 2, 2)
    calls = _record(monkeypatch, fail=(1, 3))
    with pytest.raises(RuntimeError, match="the match failed"):
        engine._error_match_gt(dp, ws)
    assert ws.err_match_gt is not None and "match indices" not in ws.valid
    engine._error_match_gt(dp, ws)
    assert len(calls) == 2 and engine._valid(ws, "match indices", ())
    engine._error_match_gt(dp, ws)
    assert len(calls) == 2


def test_detail_mode_keeps_precedence(ws, monkeypatch):
    dp = _problem("lvis", 3, 2, 2, 2)
    calls = _record(monkeypatch)
    ws.match_gt = torch.zeros((3, 20), dtype=i32)
    assert engine._error_match_gt(dp, ws) is ws.match_gt
    assert calls == [] and ws.valid == {} and ws.err_match_gt is None


def test_a_match_handed_the_workspaces_table_enters_the_product(ws, monkeypatch):
    dp = _problem("lvis", 3, 2, 2, 2)
    calls = _record(monkeypatch, name="_match", fail=(6,))
    other = torch.zeros((3, 20), dtype=i32)
    engine.stage_match(dp, ws)                                  # no table
    engine.stage_match(dp, ws, match_gt=other)                  # the caller's own
    assert len(calls) == 2 and ws.valid == {}
    own = engine.error_match_gt(dp, ws)
    engine.stage_match(dp, ws, match_gt=own)
    assert len(calls) == 3 and calls[2] is own and engine._valid(ws, "match indices", ())
    # a match that does not write the table leaves the product as it is
    engine.stage_match(dp, ws)
    engine.stage_match(dp, ws, match_gt=other)
    assert engine._valid(ws, "match indices", ())
    with pytest.raises(RuntimeError, match="the match failed"):
        engine.stage_match(dp, ws, match_gt=own)
    assert "match indices" not in ws.valid
