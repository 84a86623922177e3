"""The numpy side of the chunk tests (tests/exchange_ref.py) on its own: the
windowed run map against the reference's expression, the chunk format against
the plain statement of the result, and the condition that keeps
test_gpu_exchange_chunks.py from being vacuous -- its ground-truth counts tell
every plausible wrong run map from the true one.  No GPU, no tolerance."""
import numpy as np
import pytest

import exchange_ref
from exchange_ref import ARANGE_MAX, COUNTS, N_REC, REC_THRS, WINDOW
from exchange_ref import OFFGRID_THRS as OFFGRID, PADDED_THRS as PADDED


@pytest.mark.parametrize("thrs", [REC_THRS, PADDED, OFFGRID], ids=["default", "padded", "offgrid"])
def test_windowed_map_is_the_arange_map(thrs):
    """Window: floor(x * ng) - 3 .. + 3 (exchange_ref.WINDOW).  The crossing
    found equals the reference's for every count the arange form is used for,
    and lies strictly inside the window -- so the candidate below it was tried
    and failed, and a wider window would find the same."""
    assert WINDOW == 3 and ARANGE_MAX == 20000
    reach = 0
    for ng in range(1, ARANGE_MAX + 1):
        c, base = exchange_ref.crossings_windowed(ng, thrs, with_base=True)
        assert np.array_equal(c, exchange_ref.crossings_arange(ng, thrs)), ng
        reach = max(reach, int(np.abs(c - base).max()))
    assert reach < WINDOW, reach


def test_windowed_map_inside_its_window_at_large_counts():
    for ng in (ARANGE_MAX + 1, 65535, 65536, 10 ** 5 - 1, 10 ** 5, 10 ** 5 + 1, 10 ** 6,
               10 ** 9, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1):
        for thrs in (REC_THRS, PADDED, OFFGRID):
            c, base = exchange_ref.crossings_windowed(ng, thrs, with_base=True)
            assert int(np.abs(c - base).max()) < WINDOW, ng
            assert (c >= 0).all() and (c <= ng).all()
            assert (np.diff(c) >= 0).all()
            # the definition, at the found count and the one below it
            assert (c / np.float64(ng) >= thrs).all()
            below = np.maximum(c - 1, 0)
            assert ((below / np.float64(ng) < thrs) | (c == 0)).all()


def test_level_counts_of_the_count_list():
    for ng in COUNTS:
        nd = int(exchange_ref.run_map(ng)[-1]) + 1
        assert 1 <= nd <= min(ng, 100) + 1
        if ng > 100:
            assert nd == N_REC
    # c / 100 against the linspace bit patterns: 7 thresholds lie a rounding
    # above their j / 100 and share the next count's level
    assert int(exchange_ref.run_map(100)[-1]) + 1 == 94
    assert int(exchange_ref.run_map(1, PADDED)[-1]) + 1 == 2
    assert int(exchange_ref.run_map(2 ** 31 - 1, PADDED)[-1]) + 1 == 11


# ---- wrong run maps a kernel could plausibly compute
def _truncated(ng, thrs):
    """recall_crossing's first guess without its two fix-up loops"""
    return np.clip((thrs * np.float64(ng)).astype(np.int64), 0, ng)


def _ceil(ng, thrs):
    return np.clip(np.ceil(thrs * np.float64(ng)).astype(np.int64), 0, ng)


def _side_right(ng, thrs):
    return np.searchsorted(np.arange(ng + 1, dtype=np.float64) / ng, thrs, side="right")


def _hundredths(ng, thrs):
    """thresholds taken as j / 100.0, not as the linspace bit patterns"""
    assert thrs is REC_THRS
    j = np.arange(N_REC) / 100.0
    return (exchange_ref.crossings_arange if ng <= ARANGE_MAX
            else exchange_ref.crossings_windowed)(ng, j)


@pytest.mark.parametrize("mutant", [_truncated, _ceil, _side_right, _hundredths])
def test_count_list_tells_wrong_maps_from_the_true_one(mutant):
    caught = [ng for ng in COUNTS if ng <= ARANGE_MAX and not np.array_equal(
        exchange_ref.run_map(ng, REC_THRS, crossings=mutant), exchange_ref.run_map(ng))]
    # more than one count each, so no single row carries the whole check
    assert len(caught) >= 2, (mutant.__name__, caught)


def test_hundredths_are_not_the_threshold_bit_patterns():
    assert (np.arange(N_REC) / 100.0 != REC_THRS).sum() > 0
    assert np.array_equal(np.round(REC_THRS * 100), np.arange(N_REC))


@pytest.mark.parametrize("thrs", [REC_THRS, PADDED], ids=["default", "padded"])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_unpack_of_pack_is_expand(world, thrs):
    n_rng = 3
    n_cat = -(-2 * len(COUNTS) // n_rng)
    ng = exchange_ref.count_rows(n_cat * n_rng)
    assert set(COUNTS) <= set(ng.tolist()) and (ng == 0).sum() >= len(COUNTS)
    val, rec = exchange_ref.level_tables(ng, np.random.default_rng(world), thrs)
    Kb = -(-n_cat // world)
    table = np.zeros(world * Kb * n_rng, np.int32)
    table[:len(ng)] = ng
    cap = int(exchange_ref.sizes(Kb, n_rng, world, table, thrs).max())
    chunks = np.concatenate([exchange_ref.pack(n_cat, n_rng, Kb, b, ng, val, rec, cap, thrs)
                             for b in range(world)])
    n2, p2, r2 = exchange_ref.unpack(n_cat, n_rng, Kb, world, chunks, cap, records=True,
                                     rec_thrs=thrs)
    want_p, want_r = exchange_ref.expand(n_cat, n_rng, ng, val, rec)
    assert np.array_equal(n2.reshape(-1), ng)
    assert np.array_equal(p2, want_p)
    assert np.array_equal(r2, want_r)
    # the garbage of the dead rows is nowhere
    assert (p2[:, :, ng.reshape(n_cat, n_rng) <= 0] == -1).all()
    assert np.isfinite(p2).all() and p2.max() <= 1 and r2.max() < 1


def test_level_tables_are_valid_and_discriminating():
    ng = exchange_ref.count_rows(2 * len(COUNTS))
    val, rec = exchange_ref.level_tables(ng, np.random.default_rng(5))
    bits = val.view(np.uint64)
    for row in np.flatnonzero(ng > 0):
        d = exchange_ref.run_map(int(ng[row]))
        tp, n = bits[row] >> np.uint64(32), bits[row] & np.uint64(0xffffffff)
        assert (n >= 1).all() and (tp <= n).all()
        v = exchange_ref.decode_records(bits[row])
        same_run = d[1:] == d[:-1]
        assert (bits[row][:, 1:][:, same_run] == bits[row][:, :-1][:, same_run]).all()
        assert (v[:, 1:][:, ~same_run] != v[:, :-1][:, ~same_run]).all()
    live = bits[ng > 0]
    for tp, n in ((0, 1), (1, 1), (7, 7), (0xffffffff, 0xffffffff)):
        assert (live == np.uint64((tp << 32) | n)).any(), (tp, n)
