"""The sweep over rows the match left in CELL order, gathered through the sort's
order[] (taoamd_accumulate_by_order, _prepared, _chunked; the one-pass kernel's
gathered full-chunk loader) against the C oracle and the reference goldens, on
the cases of test_gpu_sweep_modes.py: category lengths on every boundary of the
kernels' blocking, long categories through the look-back, one and four combo
words, both row layouts, prepared and unprepared workspaces, under the look-back
and behind a counting pass; the reference fixtures and the edited-constants
goldens with every pass of the engine turned to the gathered form; the image
level's production chain (sample sort storing order[] alone, the fast match
without dst[], the gathering sweep) at a small size; and a look-back that gives
up, swept again by the chunked kernels with the rows still in cell order.
Reference: lvis_amodal/eval.py:339-426, tao_amodal/eval.py:496-584."""
import ctypes as C

import numpy as np
import pytest

import orclib
import wsguard
from goldenio import FIXTURES, load_eval, load_inputs
from tao_amodal_amd import _lib
from tao_amodal_amd import flatten as fl
from tao_amodal_amd.columns import DTColumns, GTColumns
from test_gpu_sweep_modes import SC, SIZES, _long_category_problem, _oracle_tables, _rows

pytestmark = pytest.mark.gpu

N_THR, N_REC = _lib.N_THR, _lib.N_REC
MODES = ["lookback", "twopass"]


@pytest.fixture(params=MODES)
def onepass_mode(request):
    _lib.sweep_mode(request.param)
    yield request.param
    _lib.sweep_mode("auto")


@pytest.fixture
def failing_look_back():
    _lib.sweep_mode("lookback", spin_limit=-1)
    yield
    _lib.sweep_mode("auto", spin_limit=0)


def _cell_order(seed, cat_off, whole=False):
    """order[p] = row of the sorted place p.  The match's rows of a category
    are one contiguous piece (the cells are category-major), so the realistic
    permutation shuffles inside the categories; `whole` shuffles everything."""
    rng = np.random.default_rng(seed)
    n = int(cat_off[-1])
    if whole:
        return rng.permutation(n).astype(np.int32)
    order = np.arange(n, dtype=np.int32)
    for a, b in zip(cat_off[:-1], cat_off[1:]):
        order[a:b] = a + rng.permutation(int(b - a))
    return order


def _device_tables(cat_off, matched, ignored, num_gt, order, layout, hint, how):
    """The tables of taoamd_accumulate_by_order (how = "plain"), of _prepared
    (two passes over one plan) or of _chunked, the rows stored at order[p]."""
    import torch
    lib = _lib.load()
    dev = "cuda:0"
    K, n_rng = num_gt.shape
    n, nw = matched.shape
    m_cell, i_cell = np.empty_like(matched), np.empty_like(ignored)
    m_cell[order] = matched
    i_cell[order] = ignored
    d_off = torch.from_numpy(cat_off).to(dev)
    d_ng = torch.from_numpy(num_gt).to(dev)
    d_order = torch.from_numpy(order if n else np.zeros(1, np.int32)).to(dev)
    if layout == "paired":
        rows = torch.empty((max(n, 1), nw, 2), dtype=torch.int64, device=dev)
        rows[:n, :, 0] = torch.from_numpy(m_cell.view(np.int64)).to(dev)
        rows[:n, :, 1] = torch.from_numpy(i_cell.view(np.int64)).to(dev)
        d_m, d_i = rows[..., 0], rows[..., 1]
    else:
        d_m = torch.from_numpy(np.ascontiguousarray(m_cell).view(np.int64)).to(dev)
        d_i = torch.from_numpy(np.ascontiguousarray(i_cell).view(np.int64)).to(dev)
    ws = wsguard.Guarded(lib.taoamd_accumulate_workspace(n, K, n_rng), dev)
    nbytes = ws.nbytes
    prec = torch.full((N_THR, N_REC, K, n_rng), 7.0, dtype=torch.float64, device=dev)
    rec = torch.full((N_THR, K, n_rng), 7.0, dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    args = (n, K, n_rng, d_off.data_ptr(), d_order.data_ptr(), d_m.data_ptr(), d_i.data_ptr(),
            d_ng.data_ptr(), hint, prec.data_ptr(), rec.data_ptr(), ws.data_ptr(), nbytes, s)
    if how == "prepared":
        _lib.check(lib.taoamd_accumulate_prepare(n, K, n_rng, d_off.data_ptr(), hint,
                                                 ws.data_ptr(), nbytes, s), "prepare")
        for _ in range(2):          # a prepared plan serves pass after pass
            _lib.check(lib.taoamd_accumulate_by_order_prepared(*args), "by_order_prepared")
    elif how == "chunked":
        _lib.check(lib.taoamd_accumulate_by_order_chunked(*args), "by_order_chunked")
    else:
        _lib.check(lib.taoamd_accumulate_by_order(*args), "by_order")
    flag = C.c_int32(7)
    _lib.check(lib.taoamd_accumulate_error(ws.data_ptr(), s, C.addressof(flag)), "error")
    ws.check()
    return prec.cpu().numpy(), rec.cpu().numpy(), flag.value


@pytest.mark.parametrize("layout", ["paired", "split"])
@pytest.mark.parametrize("n_rng", [6, 20])
def test_categories_on_every_boundary_of_the_blocking(onepass_mode, n_rng, layout):
    """Category lengths of 0, 1, k * 64 +- 1, k * 512 +- 1 and k * 2048 +- 1
    rows, a category that ends exactly on a super-chunk boundary followed by an
    empty one; one combo word and four; full chunks take the gathered loader,
    a category's last chunk and the split layout the generic one."""
    cat_off, m, i, ng = _rows(5 + n_rng, SIZES, n_rng)
    want_p, want_r = _oracle_tables(cat_off, m, i, ng)
    for whole in (False, True):
        order = _cell_order(17 + n_rng, cat_off, whole)
        for hint in (0, int(max(SIZES))):
            for how in ("plain", "prepared"):
                got_p, got_r, flag = _device_tables(cat_off, m, i, ng, order, layout, hint, how)
                what = (onepass_mode, n_rng, layout, whole, hint, how)
                assert flag == 0, what
                assert np.array_equal(got_r, want_r), what
                assert np.array_equal(got_p, want_p), what


def test_gathered_sweep_with_the_workspace_base_moved_by_8_bytes(onepass_mode, monkeypatch):
    monkeypatch.setattr(wsguard, "SHIFT", 8)
    test_categories_on_every_boundary_of_the_blocking(onepass_mode, 20, "paired")


@pytest.mark.parametrize("how", ["plain", "prepared"])
def test_long_categories_through_the_look_back(onepass_mode, how):
    """Categories of 40 and 70 super-chunks (the raise kernel's 64-SC rounds)
    beside short ones."""
    sizes = [40 * SC + 17, 3, 70 * SC, 0, SC]
    cat_off, m, i, ng = _rows(11, sizes, 6)
    want_p, want_r = _oracle_tables(cat_off, m, i, ng)
    order = _cell_order(23, cat_off)
    for hint in (0, int(max(sizes))):
        got_p, got_r, flag = _device_tables(cat_off, m, i, ng, order, "paired", hint, how)
        assert flag == 0
        assert np.array_equal(got_r, want_r) and np.array_equal(got_p, want_p)


def test_identity_order_is_the_streaming_sweep(onepass_mode):
    """order[p] = p: the gathered kernel over rows that are in sorted order."""
    cat_off, m, i, ng = _rows(29, SIZES, 6)
    want_p, want_r = _oracle_tables(cat_off, m, i, ng)
    order = np.arange(int(cat_off[-1]), dtype=np.int32)
    got_p, got_r, flag = _device_tables(cat_off, m, i, ng, order, "paired", 0, "prepared")
    assert flag == 0
    assert np.array_equal(got_r, want_r) and np.array_equal(got_p, want_p)


# ---------------------------------------------------------------------------
# the engine's passes turned to the gathered form
# ---------------------------------------------------------------------------
@pytest.fixture
def gathered_engine(monkeypatch):
    """Every pass the engine launches stage by stage (run_guarded: the class
    API, evaluate_flat) leaves its rows in cell order and sweeps by order[]."""
    from tao_amodal_amd import engine
    match = engine.stage_match

    def stage_match(dp, ws, scatter=True, groups=None, singles=None):
        return match(dp, ws, scatter=False, groups=groups, singles=singles)
    monkeypatch.setattr(engine, "stage_match", stage_match)
    monkeypatch.setattr(engine, "stage_accumulate", engine.stage_accumulate_by_order)
    return engine


def _gathered_pass(engine, flat, **kw):
    import torch
    dp = engine.DeviceProblem(flat, "cuda:0", **kw)
    ws = engine.Workspace(dp, keep_order=True)
    ws.precision.fill_(7.0)
    ws.recall.fill_(7.0)
    engine.run_guarded(dp, ws, flat)
    torch.cuda.synchronize()
    assert ws.cell_order and ws.sweep_recovered == 0
    # the rows are the oracle's, each where its detection is
    n = dp.n_dt
    return (ws.precision.cpu().numpy(), ws.recall.cpu().numpy(),
            ws.matched[:n].cpu().numpy().view(np.uint64),
            ws.ignored[:n].cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_goldens_through_the_gathered_sweep(onepass_mode, gathered_engine, name):
    gtj, predj = load_inputs(name)
    gt, dt = GTColumns.from_json(gtj), DTColumns.from_json(predj)
    f = fl.flatten_lvis(gt, dt)
    p, r, m, i = _gathered_pass(gathered_engine, f)
    want_p, want_r = load_eval(name)["lvis"]
    assert np.array_equal(p, want_p) and np.array_equal(r, want_r)
    want = orclib.run_flat(f, detail=False)
    assert np.array_equal(m, want["matched"]) and np.array_equal(i, want["ignored"])
    dt.track_id, _ = fl.make_track_ids_unique(dt)
    f = fl.flatten_tao(gt, dt)
    p, r, m, i = _gathered_pass(gathered_engine, f)
    want_p, want_r = load_eval(name)["tao"]
    assert np.array_equal(p.reshape(want_p.shape), want_p)
    assert np.array_equal(r.reshape(want_r.shape), want_r)
    want = orclib.run_flat(f, detail=False)
    assert np.array_equal(m, want["matched"]) and np.array_equal(i, want["ignored"])


@pytest.mark.parametrize("case", ["many", "unsorted_rec"])
@pytest.mark.parametrize("name", ["f1", "f4"])
def test_edited_constants_through_the_gathered_sweep(onepass_mode, gathered_engine, name, case):
    import test_gpu_constants as tc
    assert case in tc.cases()
    tc.test_edited_constants_match_the_reference(name, case)


# ---------------------------------------------------------------------------
# the image level's production chain at a small size
# ---------------------------------------------------------------------------
def test_the_image_level_chain_of_the_large_problems(onepass_mode, monkeypatch):
    """What run_forked launches from 6 M rows up, forced onto a small problem:
    the sample sort stores order[] and no dst[], the fast match leaves its
    rows in cell order, the prepared one-pass sweep gathers them; dst[] says
    where a detection's row is.  Alternating with the scatter form on one
    workspace."""
    import torch
    from tao_amodal_amd import engine
    monkeypatch.setattr(engine, "_SORT_FORCE", "sampled")
    _, _, f_l, _ = _long_category_problem()
    want = orclib.run_flat(f_l, detail=False)
    dp = engine.DeviceProblem(f_l, "cuda:0")
    assert engine.sort_is_sampled(dp) and engine.gathers_rows(dp)
    ws = engine.Workspace(dp)
    assert ws.gather and ws.order_buf is not None
    aux = torch.cuda.Stream("cuda:0")
    n = dp.n_dt
    for aside in (None, False, None, True):
        ws.precision.fill_(7.0)
        ws.rows.fill_(-1)
        ws.order_buf.fill_(0)
        engine.run_forked(dp, ws, aux, sort_aside=aside)
        torch.cuda.synchronize()
        assert ws.cell_order == (aside is not False)
        assert not engine.sweep_ok(dp, ws)
        assert np.array_equal(ws.precision.cpu().numpy(), want["precision"]), aside
        assert np.array_equal(ws.recall.cpu().numpy(), want["recall"]), aside
        assert np.array_equal(ws.order_buf[:n].cpu().numpy(), want["order"]), aside
        at = ws.dst[:n].long()
        assert np.array_equal(ws.matched[:n][at].cpu().numpy().view(np.uint64), want["matched"])
        assert np.array_equal(ws.ignored[:n][at].cpu().numpy().view(np.uint64), want["ignored"])
        if aside is not False:
            assert torch.equal(at, torch.arange(n, device=at.device))


# ---------------------------------------------------------------------------
# a look-back that gives up: swept again with the rows still in cell order
# ---------------------------------------------------------------------------
def test_the_flag_is_raised_and_the_chunked_entry_point_recovers(failing_look_back):
    cat_off, m, i, ng = _rows(3, SIZES, 6)
    want_p, want_r = _oracle_tables(cat_off, m, i, ng)
    order = _cell_order(31, cat_off)
    for how in ("plain", "prepared"):
        got_p, _, flag = _device_tables(cat_off, m, i, ng, order, "paired", 0, how)
        assert flag == 1                      # every look-back gave up at once
        assert not np.array_equal(got_p, want_p)
    got_p, got_r, flag = _device_tables(cat_off, m, i, ng, order, "paired", 0, "chunked")
    assert flag == 0
    assert np.array_equal(got_p, want_p) and np.array_equal(got_r, want_r)


def test_a_timed_out_gathered_pass_is_swept_again_by_the_engine(failing_look_back, monkeypatch,
                                                                caplog):
    """engine.sweep_ok behind a pass of run_forked's gathered chain: flag seen,
    chunked kernels through order[], plan rebuilt; the tables are the oracle's,
    and so are those of the next pass."""
    import torch
    from tao_amodal_amd import engine
    monkeypatch.setattr(engine, "_SORT_FORCE", "sampled")
    _, _, f_l, _ = _long_category_problem()
    want = orclib.run_flat(f_l, detail=False)
    dp = engine.DeviceProblem(f_l, "cuda:0")
    ws = engine.Workspace(dp)
    assert ws.gather
    aux = torch.cuda.Stream("cuda:0")
    for rep in range(2):
        ws.precision.fill_(7.0)
        engine.run_forked(dp, ws, aux)
        torch.cuda.synchronize()
        assert ws.cell_order
        assert engine.sweep_ok(dp, ws)
        assert ws.sweep_recovered == rep + 1
        assert np.array_equal(ws.precision.cpu().numpy(), want["precision"])
        assert np.array_equal(ws.recall.cpu().numpy(), want["recall"])
    # with the look-back working again the rebuilt plan serves the pass
    _lib.sweep_mode("lookback", spin_limit=0)
    ws.precision.fill_(7.0)
    engine.run_forked(dp, ws, aux)
    torch.cuda.synchronize()
    assert not engine.sweep_ok(dp, ws) and ws.sweep_recovered == 2
    assert np.array_equal(ws.precision.cpu().numpy(), want["precision"])
    assert any("swept again" in r.getMessage() for r in caplog.records)
