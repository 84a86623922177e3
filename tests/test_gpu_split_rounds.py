"""The sample sort's splitter kernel parks one wavefront's sorted run at a time
(four rounds over one 4 KB buffer): category sizes on both sides of every edge
that code has, score populations that drive its searches to their ends."""
import numpy as np
import pytest

import scorepop
from test_gpu_parity import _sampled_sort

pytestmark = pytest.mark.gpu

# 1024 / 1025       read directly as one bucket / split (the splitter kernel runs)
# 2816 / 2817       m = 256 / 288 samples: 1 -> 2 registers a lane
# 5632 / 5633       m = 512 / 544:  2 -> 4
# 11264 / 11265     m = 1024 / 1056: 4 -> 8
# 22528 / 22529     32 -> 16 samples a bucket (m = 2048 / 1040)
# 45056             m = 2048, every slot of the shared run in use
# 45057             two chunks and a merge pass
SIZES = [1024, 1025, 2816, 2817, 5632, 5633, 11264, 11265, 22528, 22529, 45056, 45057]
POPULATIONS = ("uniform", "ascending", "descending", "one_value", "ties", "outside")


def _layout(sizes):
    """Every size with an empty category in front of it and one at the end."""
    with_gaps = [0]
    for s in sizes:
        with_gaps += [s, 0]
    cat_off = np.zeros(len(with_gaps) + 1, np.int32)
    np.cumsum(with_gaps, out=cat_off[1:])
    return cat_off


def _scores(kind, cat_off, rng):
    n = int(cat_off[-1])
    cat = np.repeat(np.arange(len(cat_off) - 1), np.diff(cat_off))
    within = np.arange(n) - cat_off[cat]
    if kind == "uniform":
        return rng.random(n)
    if kind == "ascending":
        # already in order one way or the other: the 64-sample blocks of the
        # four wavefronts' runs are disjoint ranges of values, so a search
        # ends at 0 or at the run's length wherever it can
        return within / 65536.0
    if kind == "descending":
        return -within / 65536.0
    if kind == "one_value":
        return np.full(n, 0.125)                 # ordered by the position bits alone
    if kind == "ties":
        s = rng.random(n)
        s[rng.random(n) < 0.3] = 0.5
        return s
    assert kind == "outside", kind
    s = scorepop.score_population("nan", n, rng, cat_off)
    special = rng.random(n) < 0.2                # +-inf, +-0, subnormals, +-DBL_MAX
    s[special] = scorepop.score_population("specials", n, rng)[special]
    assert np.isnan(s).any() and np.isinf(s).any()
    return s


@pytest.mark.parametrize("limit", [0, 300])
@pytest.mark.parametrize("kind", POPULATIONS)
def test_split_rounds_every_edge(kind, limit):
    """All sizes in one launch sequence, run twice on one workspace.  limit =
    300: buckets beyond 300 elements take the overflow path (the sizes up to
    5633)."""
    import torch
    from tao_amodal_amd import _lib
    lib = _lib.load()
    sizes = [s for s in SIZES if s <= 5633] if limit else SIZES
    cat_off = _layout(sizes)
    n, n_cat = int(cat_off[-1]), len(cat_off) - 1
    rng = np.random.default_rng([10, POPULATIONS.index(kind), limit])
    score = _scores(kind, cat_off, rng)
    cat = np.repeat(np.arange(n_cat), np.diff(cat_off))
    want = np.lexsort((np.arange(n), -score, cat))
    tiles = (np.diff(cat_off) + _lib.SEGMENT_TILE - 1) // _lib.SEGMENT_TILE
    tile_off = np.zeros(n_cat + 1, np.int32)
    np.cumsum(tiles, out=tile_off[1:])
    d_score = torch.from_numpy(score).cuda()
    try:
        lib.taoamd_sort_sampled_cap_limit(limit)
        order, dst = _sampled_sort(cat_off, tile_off, d_score, repeat=2)
    finally:
        lib.taoamd_sort_sampled_cap_limit(0)
    assert np.array_equal(order, want)
    assert np.array_equal(dst[want], np.arange(n))
