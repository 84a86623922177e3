"""-m gpu: taoamd_exchange_{sizes,pack,unpack} (csrc/exchange.hip) on tables
written by the test itself, at every ground-truth count, scan share and unpack
tile edge, against tests/exchange_ref.py.  No evaluation runs: num_gt, val and
rec are plain tables (exchange_ref.level_tables), so the counts reach 2^31 - 1
and the shapes the edges of the kernels while the cases stay small.

Everything is compared with np.array_equal: the records travel untouched and
tp / (n + eps) is one correctly rounded division on both sides.  That the
counts used tell a wrong run map from the true one is shown on the CPU
(test_exchange_ref_host.py)."""
import numpy as np
import pytest

import exchange_ref
import wsguard
from exchange_ref import COUNTS, N_REC, N_THR, OFFGRID_THRS, PADDED_THRS, REC_THRS

pytestmark = pytest.mark.gpu

DEV = "cuda"
BIG = 2 ** 31 - 1


def _backend():
    from tao_amodal_amd import dist
    return dist.HipBackend()


def _set_rec_thrs(thrs=None):
    from tao_amodal_amd import _lib
    _lib.set_constants(rec_thrs=thrs)


def _typed(shape, dtype, fill):
    """A tensor in a guarded buffer of exactly its size, filled with `fill`."""
    import torch
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    g = wsguard.Guarded(nbytes, device=DEV, shift=0)
    t = g.tensor.view(dtype).view(*shape)
    t.fill_(fill)
    return g, t


def _first_diff(got, want):
    bad = np.flatnonzero(got != want)
    return (len(bad), int(bad[0]) if len(bad) else None)


def _chunk_levels(chunk, block_rows, total):
    """(num_gt, levels) of the live rows of a chunk, from its header alone"""
    h = chunk[:block_rows * 4].view(np.int32)
    ho = chunk[block_rows * 4:block_rows * 8].view(np.int32)
    live = np.flatnonzero(h > 0)
    ends = np.r_[ho[live][1:], total].astype(np.int64)
    nd = (ends - ho[live]) // N_THR
    assert ((ends - ho[live]) % N_THR == 0).all()
    return h[live], nd


def _exchange(n_cat, n_rng, Kb, world, ng, val, rec, thrs=REC_THRS, maps_ready=False,
              null_out=False):
    """sizes, pack of every rank, unpack; the assertions every case makes.
    maps_ready: pack and unpack take the maps and offsets the _sizes call left
    in its workspace; otherwise they build their own on a second workspace
    that holds a byte pattern.  -> what the device produced."""
    import torch
    be = _backend()
    KR, BR = n_cat * n_rng, Kb * n_rng
    assert Kb * world >= n_cat
    ng = np.ascontiguousarray(ng, dtype=np.int32).reshape(n_cat, n_rng)
    val = np.ascontiguousarray(val).reshape(n_cat, n_rng, N_THR, N_REC)
    rec = np.ascontiguousarray(rec).reshape(n_cat, n_rng, N_THR)
    table = np.zeros((world * Kb, n_rng), np.int32)
    table.reshape(-1)[:KR] = ng.reshape(-1)
    d_ng, d_table = torch.from_numpy(ng).to(DEV), torch.from_numpy(table).to(DEV)
    d_val, d_rec = torch.from_numpy(val).to(DEV), torch.from_numpy(rec).to(DEV)

    ws_bytes = be.exchange_workspace(Kb, n_rng, world)
    w1 = wsguard.Guarded(ws_bytes, device=DEV)
    totals = torch.full((world,), -1, dtype=torch.int64, device=DEV)
    be.exchange_sizes(Kb, n_rng, world, d_table, totals, w1.tensor)
    w1.check()
    want_sizes = exchange_ref.sizes(Kb, n_rng, world, table, thrs)
    totals = totals.cpu().numpy()
    assert np.array_equal(totals, want_sizes)
    cap = int(want_sizes.max())
    cb = be.exchange_chunk_bytes(Kb, n_rng, cap)
    assert cb == exchange_ref.layout(Kb, n_rng, cap)[2]

    wx = w1 if maps_ready else wsguard.Guarded(ws_bytes, device=DEV)
    og, over = _typed((1,), torch.int32, 0)
    allg = wsguard.Guarded(world * cb, device=DEV)
    for b in range(world):
        cg = wsguard.Guarded(cb, device=DEV)
        cg.tensor.zero_()
        be.exchange_pack(n_cat, n_rng, Kb, world, b, d_ng, d_val, d_rec, cg.tensor, cap,
                         None if null_out else over, wx.tensor, maps_ready)
        cg.check()
        wx.check()
        got = cg.tensor.cpu().numpy()
        want = exchange_ref.pack(n_cat, n_rng, Kb, b, ng, val, rec, cap, thrs)
        assert np.array_equal(got, want), (b, _first_diff(got, want))
        allg.tensor[b * cb:(b + 1) * cb] = cg.tensor
    chunks = allg.tensor.cpu().numpy()

    pg, prec = _typed((N_THR, N_REC, n_cat, n_rng), torch.float64, 7.0)
    rg, rcl = _typed((N_THR, n_cat, n_rng), torch.float64, 7.0)
    ngg, ngo = _typed((n_cat, n_rng), torch.int32, 77)
    be.exchange_unpack(n_cat, n_rng, Kb, world, allg.tensor, cap,
                       None if null_out else ngo, prec, rcl, None if null_out else over,
                       wx.tensor, maps_ready)
    for g in (wx, allg, pg, rg, ngg, og):
        g.check()
    assert np.array_equal(allg.tensor.cpu().numpy(), chunks)      # unpack only reads
    assert int(over.item()) == 0
    prec, rcl, ngo = prec.cpu().numpy(), rcl.cpu().numpy(), ngo.cpu().numpy()
    want_p, want_r = exchange_ref.expand(n_cat, n_rng, ng, val, rec)
    if null_out:
        assert (ngo == 77).all()
    else:
        assert np.array_equal(ngo, ng)
    assert np.array_equal(prec, want_p), _first_diff(prec.reshape(-1), want_p.reshape(-1))
    assert np.array_equal(rcl, want_r), _first_diff(rcl.reshape(-1), want_r.reshape(-1))
    n2, p2, r2 = exchange_ref.unpack(n_cat, n_rng, Kb, world, chunks, cap, records=True,
                                     rec_thrs=thrs)
    assert np.array_equal(n2, ng) and np.array_equal(p2, prec) and np.array_equal(r2, rcl)
    return dict(totals=totals, cap=cap, chunk_bytes=cb, chunks=chunks, num_gt=ngo,
                precision=prec, recall=rcl)


# ---- A. count edges
@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("n_rng", [1, 6, 20])
def test_count_edges(n_rng, world):
    """Every count of exchange_ref.COUNTS (1 .. 2^31 - 1, both sides of 50, 100
    and 200) in one table, zeros between them."""
    n_cat = -(-2 * len(COUNTS) // n_rng)
    ng = exchange_ref.count_rows(n_cat * n_rng)
    assert set(COUNTS) <= set(ng.tolist())
    val, rec = exchange_ref.level_tables(ng, np.random.default_rng(100 * n_rng + world))
    Kb = -(-n_cat // world)
    out = _exchange(n_cat, n_rng, Kb, world, ng, val, rec)
    seen = {}
    for b in range(world):
        c = out["chunks"][b * out["chunk_bytes"]:(b + 1) * out["chunk_bytes"]]
        for n, nd in zip(*_chunk_levels(c, Kb * n_rng, int(out["totals"][b]))):
            assert 1 <= nd <= min(int(n), 100) + 1, (int(n), int(nd))
            seen[int(n)] = int(nd)
    assert set(seen) == set(COUNTS)
    assert seen[100] == 94       # not 101: c / 100 against the linspace bit patterns
    assert seen[1] == 2 and seen[101] == 101 and seen[BIG] == 101


# ---- B. scan edges
SCAN_SHAPES = [(1, 1), (63, 1), (2, 32), (65, 1), (1023, 1), (32, 32), (1025, 1), (2047, 1),
               (64, 32), (2049, 1), (151, 20)]       # (block_cats, n_rng)
SCAN_PATTERNS = ["live", "last", "dead64", "deadshare", "deadshares", "alt"]


def _share(BR):
    """rows one of the 16 wavefronts of ex_offsets_kernel scans"""
    return ((BR + 15) // 16 + 63) // 64 * 64


def _dead_rows(pattern, BR):
    """Leading rows without ground truth: one 64-row step; the whole share of
    wavefront 0 (its total is 0, and so is the base of wavefront 1); two
    shares and a step."""
    per = _share(BR)
    return {"dead64": 64, "deadshare": per, "deadshares": 2 * per + 64}[pattern]


def _scan_cases():
    out = []
    for bc, r in SCAN_SHAPES:
        seen = set()
        for p in SCAN_PATTERNS:
            if p.startswith("dead"):
                dead = _dead_rows(p, bc * r)
                if dead >= bc * r or dead in seen:      # no live row left / the same case
                    continue
                seen.add(dead)
            out.append((bc, r, p))
    return out


def _scan_counts(pattern, BR, block, rng):
    """num_gt of one block's rows"""
    live = rng.choice(np.array(COUNTS, dtype=np.int64), BR)
    if pattern == "live":
        return live
    if pattern == "last":
        out = np.zeros(BR, np.int64)
        out[-1] = (BIG, 1)[block]
        return out
    if pattern == "alt":
        return np.array([0, 1, BIG], dtype=np.int64)[(np.arange(BR) + block) % 3]
    dead = _dead_rows(pattern, BR)
    if block == 0:
        live[:dead] = 0
    else:                       # the second block has them at its tail
        live[BR - dead:] = 0
    return live


def test_scan_shapes_are_the_edges():
    sizes = sorted(bc * r for bc, r in SCAN_SHAPES)
    assert sizes == [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3020]
    assert {r for _, r in SCAN_SHAPES} == {1, 20, 32}
    # the share changes where the issue says it does
    assert [_share(n) for n in sizes] == [64] * 6 + [128] * 3 + [192] * 2
    cases = _scan_cases()
    for bc, r in SCAN_SHAPES:
        assert {p for b, q, p in cases if (b, q) == (bc, r)} >= {"live", "last", "alt"}
    assert sum(p.startswith("dead") for _, _, p in cases) == 5 + 3 * 5


@pytest.mark.parametrize("block_cats,n_rng,pattern", _scan_cases())
def test_scan_edges(block_cats, n_rng, pattern):
    world, BR = 2, block_cats * n_rng
    rng = np.random.default_rng(BR * 10 + SCAN_PATTERNS.index(pattern))
    ng = np.concatenate([_scan_counts(pattern, BR, b, rng) for b in range(world)])
    val, rec = exchange_ref.level_tables(ng, rng)
    _exchange(world * block_cats, n_rng, block_cats, world, ng, val, rec)


# ---- C. unpack tile edges
TILE_SHAPES = [(1, 1, 1), (7, 9, 3), (2, 32, 1), (64, 1, 22), (5, 13, 2), (127, 1, 43),
               (43, 3, 15), (101, 10, 34), (505, 2, 253)]      # (n_cat, n_rng, block_cats)


def _tile_counts(KR, pattern, rng):
    ng = rng.choice(np.array(COUNTS + (0,) * 10, dtype=np.int64), KR)
    if pattern == "deadtile":
        # an aligned run of dead rows: a tile without a live row between live ones
        ng[64:128] = 0
        ng[63] = 3
        if KR > 128:
            ng[128] = 100
    return ng


def test_tile_shapes_are_the_edges():
    assert sorted({k * r for k, r, _ in TILE_SHAPES}) == [1, 63, 64, 65, 127, 129, 1010]
    for n_cat, n_rng, Kb in TILE_SHAPES:
        assert (Kb * n_rng) % 64 != 0 and n_cat % 3 != 0 and Kb * 3 >= n_cat
    # last block all padding
    assert sum(2 * Kb >= n_cat for n_cat, _, Kb in TILE_SHAPES) >= 3


@pytest.mark.parametrize("pattern", ["mixed", "deadtile"])
@pytest.mark.parametrize("n_cat,n_rng,block_cats", TILE_SHAPES)
def test_unpack_tile_edges(n_cat, n_rng, block_cats, pattern):
    KR = n_cat * n_rng
    if pattern == "deadtile" and KR <= 64:
        return _all_dead(n_cat, n_rng, block_cats)
    rng = np.random.default_rng(KR + 7 * n_rng + (pattern == "deadtile"))
    ng = _tile_counts(KR, pattern, rng)
    val, rec = exchange_ref.level_tables(ng, rng)
    _exchange(n_cat, n_rng, block_cats, 3, ng, val, rec)


def _all_dead(n_cat, n_rng, block_cats):
    """no ground truth anywhere: capacity 0, every cell -1"""
    ng = np.zeros(n_cat * n_rng, np.int32)
    val, rec = exchange_ref.level_tables(ng, np.random.default_rng(1))
    out = _exchange(n_cat, n_rng, block_cats, 3, ng, val, rec)
    assert out["cap"] == 0
    assert (out["precision"] == -1).all() and (out["recall"] == -1).all()


def test_unpack_without_optional_outputs():
    """num_gt_out = NULL and overflow = NULL (pack's too)"""
    n_cat, n_rng, Kb = 43, 3, 15
    rng = np.random.default_rng(9)
    ng = _tile_counts(n_cat * n_rng, "deadtile", rng)
    val, rec = exchange_ref.level_tables(ng, rng)
    _exchange(n_cat, n_rng, Kb, 3, ng, val, rec, null_out=True)


# ---- D. maps_ready
def test_maps_ready_equals_own_maps():
    """The by-video plan's path: maps and offsets from one _sizes call on the
    table of all rows, pack and unpack with maps_ready = 1."""
    n_cat, n_rng, Kb, world = 103, 20, 52, 2        # block_rows 1040, one padding category
    ng = exchange_ref.count_rows(n_cat * n_rng)
    val, rec = exchange_ref.level_tables(ng, np.random.default_rng(4))
    ready = _exchange(n_cat, n_rng, Kb, world, ng, val, rec, maps_ready=True)
    own = _exchange(n_cat, n_rng, Kb, world, ng, val, rec, maps_ready=False)
    for key in ("totals", "chunks", "num_gt", "precision", "recall"):
        assert np.array_equal(ready[key], own[key]), key


# ---- E. capacity
@pytest.mark.parametrize("count,live", [(1, 8), (BIG, 16), (100, 16)])
def test_capacity_one_level_short(count, live):
    """A block that needs L levels with capacity L - 1: pack reports it and
    writes nothing behind the smaller chunk, unpack reports it; every cell but
    the run of the level that is missing is still right."""
    import torch
    be = _backend()
    n_cat = Kb = 2 * live
    n_rng = world = 1
    ng = np.zeros(n_cat, np.int32)
    ng[::2] = count
    val, rec = exchange_ref.level_tables(ng, np.random.default_rng(live))
    L = int(exchange_ref.sizes(Kb, n_rng, world, ng)[0])
    cap = L - 1
    cb = be.exchange_chunk_bytes(Kb, n_rng, cap)
    hdr, recb, total = exchange_ref.layout(Kb, n_rng, cap)
    # L is even and the levels are padded to 256 bytes, so the short chunk is
    # as large as the full one: the level that does not fit would land in the
    # padding behind the levels, which must stay as it was
    assert cb == total and hdr + recb + cap * 8 < cb
    d_ng = torch.from_numpy(ng.reshape(n_cat, 1)).to(DEV)
    d_val = torch.from_numpy(val.reshape(n_cat, 1, N_THR, N_REC)).to(DEV)
    d_rec = torch.from_numpy(rec.reshape(n_cat, 1, N_THR)).to(DEV)
    ws = wsguard.Guarded(be.exchange_workspace(Kb, n_rng, world), device=DEV)
    og, over = _typed((1,), torch.int32, 0)
    want = exchange_ref.pack(n_cat, n_rng, Kb, 0, ng, val, rec, L)[:hdr + recb + cap * 8]
    chunks = []
    for flag in (over, None):        # overflow = NULL: the call is still OK
        cg = wsguard.Guarded(cb, device=DEV)
        cg.tensor.zero_()
        be.exchange_pack(n_cat, n_rng, Kb, world, 0, d_ng, d_val, d_rec, cg.tensor, cap,
                         flag, ws.tensor)
        cg.check()
        ws.check()
        og.check()
        got = cg.tensor.cpu().numpy()
        assert np.array_equal(got[:len(want)], want) and not got[len(want):].any()
        chunks.append(cg)
    assert int(over.item()) == 1
    # with room for all levels the flag stays clear
    over.zero_()
    full = wsguard.Guarded(be.exchange_chunk_bytes(Kb, n_rng, L), device=DEV)
    full.tensor.zero_()
    be.exchange_pack(n_cat, n_rng, Kb, world, 0, d_ng, d_val, d_rec, full.tensor, L, over,
                     ws.tensor)
    full.check()
    assert int(over.item()) == 0
    assert np.array_equal(full.tensor.cpu().numpy(),
                          exchange_ref.pack(n_cat, n_rng, Kb, 0, ng, val, rec, L))

    want_p, want_r = exchange_ref.expand(n_cat, n_rng, ng, val, rec)
    lost = np.zeros(want_p.shape, bool)         # the last level: threshold 9, last run
    d = exchange_ref.run_map(count)
    lost[N_THR - 1, d == d[-1], n_cat - 2, 0] = True
    for flag in (over, None):
        pg, prec = _typed((N_THR, N_REC, n_cat, n_rng), torch.float64, 7.0)
        rg, rcl = _typed((N_THR, n_cat, n_rng), torch.float64, 7.0)
        ngg, ngo = _typed((n_cat, n_rng), torch.int32, 77)
        be.exchange_unpack(n_cat, n_rng, Kb, world, chunks[0].tensor, cap, ngo, prec, rcl,
                           flag, ws.tensor)
        for g in (ws, chunks[0], pg, rg, ngg, og):
            g.check()
        prec = prec.cpu().numpy()
        assert np.array_equal(prec[~lost], want_p[~lost])
        assert np.array_equal(rcl.cpu().numpy(), want_r)
        assert np.array_equal(ngo.cpu().numpy().reshape(-1), ng)
    assert int(over.item()) == 1


def test_block_without_ground_truth():
    """A zero-level chunk beside full ones unpacks to -1 rows."""
    n_cat, n_rng, Kb, world = 6, 4, 2, 3
    ng = exchange_ref.count_rows(n_cat * n_rng, COUNTS[5:]).reshape(n_cat, n_rng)
    ng[2:4] = 0
    val, rec = exchange_ref.level_tables(ng, np.random.default_rng(2))
    out = _exchange(n_cat, n_rng, Kb, world, ng, val, rec)
    assert out["totals"][1] == 0 and out["totals"][0] > 0 and out["totals"][2] > 0
    assert (out["precision"][:, :, 2:4] == -1).all() and (out["recall"][:, 2:4] == -1).all()


def test_no_ground_truth_at_all():
    _all_dead(5, 13, 2)


# ---- F. edited recall thresholds
@pytest.mark.parametrize("name", ["padded", "offgrid"])
def test_edited_recall_thresholds(name):
    """The run maps follow the calling thread's thresholds
    (taoamd_set_thresholds): a shorter list padded with its last value has at
    most 11 levels whatever num_gt, one off the hundredths other collisions."""
    thrs = {"padded": PADDED_THRS, "offgrid": OFFGRID_THRS}[name]
    assert thrs.min() >= 0 and thrs.max() <= 1
    assert any(not np.array_equal(exchange_ref.run_map(n, thrs), exchange_ref.run_map(n))
               for n in COUNTS)
    n_cat, n_rng, Kb, world = 25, 2, 13, 2
    ng = exchange_ref.count_rows(n_cat * n_rng)
    val, rec = exchange_ref.level_tables(ng, np.random.default_rng(3), thrs)
    _set_rec_thrs(thrs)
    try:
        out = _exchange(n_cat, n_rng, Kb, world, ng, val, rec, thrs)
    finally:
        _set_rec_thrs()
    if name == "padded":
        assert out["cap"] <= Kb * n_rng * 11 * N_THR
    # the defaults are back
    val, rec = exchange_ref.level_tables(ng, np.random.default_rng(3))
    _exchange(n_cat, n_rng, Kb, world, ng, val, rec)
