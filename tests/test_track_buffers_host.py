"""No GPU: the two host rules of the track analyses' stages on a bare workspace
(engine._buffer, engine._workspace; engine._valid, engine._producing), with CPU
tensors."""
import pytest
import torch

from tao_amodal_amd import engine

CPU = torch.device("cpu")


@pytest.fixture
def ws():
    w = object.__new__(engine.Workspace)
    w.declare_track_products()
    return w


def test_every_track_product_is_declared_once(ws):
    names = engine.Workspace.TRACK_PRODUCTS
    assert len(set(names)) == len(names)
    assert all(getattr(ws, n) is None for n in names) and ws.valid == {}


def test_at_least_rule(ws):
    a = engine._buffer(ws, CPU, "hota_mc", (3, 5), torch.int32)
    assert a.shape == (3, 5) and a.dtype == torch.int32 and a.is_contiguous()
    assert ws.hota_mc.data_ptr() == a.data_ptr()
    held = ws.hota_mc
    b = engine._buffer(ws, CPU, "hota_mc", (3, 5), torch.int32)
    assert ws.hota_mc is held and b.data_ptr() == a.data_ptr()       # the same storage
    # a smaller request: the larger buffer stays and is handed out; the leading rows are
    # a contiguous view at its address
    c = engine._buffer(ws, CPU, "hota_mc", (2, 5), torch.int32)
    assert ws.hota_mc is held and c is held
    assert c[:2].shape == (2, 5) and c[:2].data_ptr() == a.data_ptr() and c[:2].is_contiguous()
    # a larger one regrows it; so does another trailing shape
    d = engine._buffer(ws, CPU, "hota_mc", (4, 5), torch.int32)
    assert ws.hota_mc is not held and ws.hota_mc.shape == (4, 5) and d.shape == (4, 5)
    held = ws.hota_mc
    e = engine._buffer(ws, CPU, "hota_mc", (1, 6), torch.int32)
    assert ws.hota_mc is not held and ws.hota_mc.shape == (1, 6) and e.shape == (1, 6)
    # an int is a one-dimensional shape
    f = engine._buffer(ws, CPU, "clear_row", 7, torch.float64)
    assert f.shape == (7,) and f.dtype == torch.float64
    assert engine._buffer(ws, CPU, "clear_row", 4, torch.float64) is f and ws.clear_row is f


def test_exact_rule(ws):
    a = engine._buffer(ws, CPU, "assoc_vis_counts", (2, 4, 3), torch.int64, exact=True)
    assert a is ws.assoc_vis_counts and a.shape == (2, 4, 3) and a.dtype == torch.int64
    assert engine._buffer(ws, CPU, "assoc_vis_counts", (2, 4, 3), torch.int64, exact=True) is a
    # a different shape, smaller or larger: a buffer of that shape
    b = engine._buffer(ws, CPU, "assoc_vis_counts", (1, 4, 3), torch.int64, exact=True)
    assert b is not a and b is ws.assoc_vis_counts and b.shape == (1, 4, 3)
    c = engine._buffer(ws, CPU, "assoc_vis_counts", (5, 4, 3), torch.int64, exact=True)
    assert c is ws.assoc_vis_counts and c.shape == (5, 4, 3)
    # no windows: no table
    assert engine._buffer(ws, CPU, "assoc_vis_counts", (0, 4, 3), torch.int64, exact=True) is None
    assert ws.assoc_vis_counts is None
    d = engine._buffer(ws, CPU, "assoc_vis_counts", (5, 4, 3), torch.int64, exact=True)
    assert d is ws.assoc_vis_counts and d.shape == (5, 4, 3)


def test_workspace_pair(ws):
    engine._workspace(ws, CPU, "occ", 100)
    assert ws.occ_bytes == 100 and ws.occ_ws.numel() == 256 and ws.occ_ws.dtype == torch.uint8
    held = ws.occ_ws
    engine._workspace(ws, CPU, "occ", 100)
    assert ws.occ_ws is held and ws.occ_bytes == 100
    engine._workspace(ws, CPU, "occ", 40)                            # the larger one stays
    assert ws.occ_ws is held and ws.occ_bytes == 100
    engine._workspace(ws, CPU, "occ", 1000)
    assert ws.occ_bytes == 1000 and ws.occ_ws.numel() == 1000 and ws.occ_ws is not held


def test_product_rule(ws):
    assert not engine._valid(ws, "followers", 0.5)
    ran = []
    with engine._producing(ws, "followers", 0.5):
        assert not engine._valid(ws, "followers", 0.5)              # not before it is through
        ran.append(0.5)
    assert ran == [0.5] and engine._valid(ws, "followers", 0.5)
    assert not engine._valid(ws, "followers", 0.75)                 # a different key
    assert not engine._valid(ws, "identity", 0.5)                   # a different product
    with engine._producing(ws, "identity", 0.75):
        pass
    assert engine._valid(ws, "followers", 0.5) and engine._valid(ws, "identity", 0.75)
    # a producer that raises leaves the product valid for no key, not even the one before
    with pytest.raises(RuntimeError, match="midway"):
        with engine._producing(ws, "followers", 0.75):
            raise RuntimeError("midway")
    assert not engine._valid(ws, "followers", 0.75) and not engine._valid(ws, "followers", 0.5)
    assert "followers" not in ws.valid and engine._valid(ws, "identity", 0.75)
    with engine._producing(ws, "followers", 0.75):
        pass
    assert engine._valid(ws, "followers", 0.75)
