"""The compact sweep's plane form (csrc/accumulate.hip, crow_pack / crow_planes).

A full 512-row chunk of 4-byte match rows is no longer expanded row by row:
the 18 bits of three 64-row blocks are packed into one 64-bit word a lane,
w0 | w1 << 18 | w2 << 36, ONE 64 x 64 transpose leaves the 64-row plane of bit p
of block j in lane 18 j + p, and combo lane (a, t) puts its two words together
from four planes,
    T  = P_t & ~(G_a | H)                          (TP)
    TF = (P_t & ~(G_a | (H & U))) | (~P_t & ~U)    (valid)
with P_t, G_a, U, H the planes of bits t, 10 + a, 16 and 17.  A partial chunk (a
category's last) and a block with an escaped word keep the table form.

Checked here: the formulas and the packed-and-transposed layout against the
match kernel's products over all 2^18 words (host, numpy); that the inputs of
the every-word test leave no bit free (host, the C oracle: one flipped TP or
valid bit in a category's last block changes the tables); every word through
the compact sweep against the 16-byte gathered instance and the oracle; and the
blocking edges -- the group edges at 192 and 384 rows among them -- with escaped
rows in every position a block can meet them.
Reference: lvis_amodal/eval.py:339-426 (accumulate)."""
import functools

import numpy as np
import pytest

from tao_amodal_amd import _lib
from test_gpu_compact_rows import CHUNK, ESCAPE, SC, U64, _compact_tables, expand_products

gpu = pytest.mark.gpu

N_THR, N_REC = _lib.N_THR, _lib.N_REC
WAVE = 64
BITS = 18                       # bits of a word that say something
GROUP = 3                       # blocks to a transpose


# ---------------------------------------------------------------------------
# the plane form, in numpy
# ---------------------------------------------------------------------------
def transpose64(rows):
    """rows[..., i] = row i of a 64 x 64 bit matrix (bit j = element (i, j));
    out[..., j] = column j (bit i = element (i, j))."""
    rows = np.asarray(rows, U64)
    out = np.zeros(rows.shape, U64)
    for i in range(WAVE):
        bit_j = (rows[..., i, None] >> np.arange(WAVE, dtype=U64)) & U64(1)
        out |= bit_j << U64(i)
    return out


def plane_words(w, n_rng):
    """(T, TF) of the 64-row blocks of the words w, lane by lane, as the plane
    path builds them: (blocks, 64) each.  len(w) is a multiple of 64."""
    w = np.asarray(w, np.uint32).reshape(-1, WAVE)
    nb = len(w)
    pad = (-nb) % GROUP
    w = np.concatenate([w, np.zeros((pad, WAVE), np.uint32)])
    m = (w & np.uint32((1 << BITS) - 1)).astype(U64).reshape(-1, GROUP, WAVE)
    packed = m[:, 0] | m[:, 1] << U64(BITS) | m[:, 2] << U64(2 * BITS)
    X = transpose64(packed)                                # (groups, 64 lanes)
    lane = np.arange(WAVE)
    t, a = lane % N_THR, lane // N_THR                     # (lanes 60-63: a = 6, dead)
    dead = lane >= n_rng * N_THR
    T, TF = [], []
    for j in range(GROUP):
        # the plane of bit p of block j sits in lane 18 j + p
        P, G = X[:, BITS * j + t], X[:, BITS * j + N_THR + a]
        U, H = X[:, BITS * j + 16, None], X[:, BITS * j + 17, None]
        T.append(np.where(dead, U64(0), P & ~(G | H)))
        TF.append((P & ~(G | (H & U))) | (~P & ~U))
    T = np.stack(T, 1).reshape(-1, WAVE)[:nb]
    TF = np.stack(TF, 1).reshape(-1, WAVE)[:nb]
    return T, TF


@functools.lru_cache(maxsize=None)
def _all_words(seed, junk):
    """Every 18-bit word once, in a seeded permutation; junk: anything in bits
    18-30 (a plain word's bit 31 is clear)."""
    rng = np.random.default_rng(seed)
    w = rng.permutation(1 << BITS).astype(np.uint32)
    if junk:
        w |= rng.integers(0, 1 << 13, len(w)).astype(np.uint32) << np.uint32(BITS)
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("junk", [False, True])
def test_the_plane_form_equals_the_products_over_all_words(junk):
    """All 2^18 words, one to six ranges, packed three blocks to a word and
    transposed as the kernel does: T = the transposed matched & ~ignored in
    every lane (zero above the ranges' combos), TF = the transposed ~ignored in
    the ranges' lanes."""
    w = _all_words(5, junk)
    for n_rng in range(1, 7):
        m, i = expand_products(w, n_rng)
        want_t = transpose64((m & ~i).reshape(-1, WAVE))
        want_v = transpose64((~i).reshape(-1, WAVE))
        T, TF = plane_words(w, n_rng)
        live = n_rng * N_THR
        assert np.array_equal(T, want_t), n_rng
        assert not T[:, live:].any(), n_rng
        assert np.array_equal(TF[:, :live], want_v[:, :live]), n_rng


def test_the_packed_word_puts_plane_p_of_block_j_in_lane_18j_plus_p():
    rng = np.random.default_rng(2)
    w = rng.integers(0, 1 << 31, (GROUP, WAVE)).astype(np.uint32)
    m = (w & np.uint32((1 << BITS) - 1)).astype(U64)
    X = transpose64(m[0] | m[1] << U64(BITS) | m[2] << U64(2 * BITS))
    for j in range(GROUP):
        for p in range(BITS):
            plane = sum(((int(w[j, i]) >> p) & 1) << i for i in range(WAVE))
            assert int(X[BITS * j + p]) == plane, (j, p)
    assert not X[GROUP * BITS:].any()


# ---------------------------------------------------------------------------
# every word
# ---------------------------------------------------------------------------
# three categories of unequal length: the first ends on a super-chunk boundary
# (its last chunk is a full one: planes), the others in a block of 32 rows
EVERY_SIZES = (49 * SC, 98784, (1 << BITS) - 49 * SC - 98784)
EVERY_INPUTS = [(11, False), (12, False), (13, False), (14, True)]


def _oracle(cat_off, matched, ignored, num_gt):
    from test_gpu_sweep_modes import _oracle_tables
    return _oracle_tables(cat_off, matched, ignored, num_gt)


@functools.lru_cache(maxsize=None)
def _every_word_case(seed, junk, n_rng):
    """The words, their rows, and num_gt[k][r] = the largest TP total of the
    range's ten thresholds.  The threshold whose total that is reaches recall
    1.0 on its last TP row -- in the category's last block or next to it (one
    row in eight is a TP) -- and the others cross their last recall threshold
    within num_gt / 100 TPs of their end, about 900 rows: every lane's counts
    are still being read in the last 2 048 rows of every category."""
    words = _all_words(seed, junk)
    n = len(words)
    cat_off = np.zeros(len(EVERY_SIZES) + 1, np.int32)
    np.cumsum(EVERY_SIZES, out=cat_off[1:])
    assert cat_off[-1] == n
    m, i = expand_products(words, n_rng)
    matched, ignored = m[:, None].copy(), i[:, None].copy()
    tp = m & ~i
    num_gt = np.zeros((len(EVERY_SIZES), n_rng), np.int32)
    for k in range(len(EVERY_SIZES)):
        a, b = cat_off[k], cat_off[k + 1]
        for r in range(n_rng):
            num_gt[k, r] = max(int(((tp[a:b] >> U64(N_THR * r + t)) & U64(1)).sum())
                               for t in range(N_THR))
    assert (num_gt > 0).all()
    rng = np.random.default_rng(seed + 100)
    order = np.arange(n, dtype=np.int32)          # shuffled inside the categories
    for a, b in zip(cat_off[:-1], cat_off[1:]):
        order[a:b] = a + rng.permutation(int(b - a))
    want_p, want_r = _oracle(cat_off, matched, ignored, num_gt)
    return (cat_off, words, matched, ignored, num_gt, order, np.zeros(n, bool),
            want_p, want_r)


@pytest.mark.parametrize("seed,junk", EVERY_INPUTS)
def test_one_flipped_bit_in_a_last_block_changes_the_oracles_tables(seed, junk):
    """The condition that makes the every-word test conclusive, on the oracle
    alone (the seeds were chosen for it): in each category's last 64-row block
    a row's TP bit flipped (the row stays valid) changes the tables -- a lane's
    recall is its TP total over num_gt, so this holds in any lane; one lane a
    range is run --, and a valid bit flipped (a false positive more or less) changes
    them in every range: in the lane that reaches recall 1.0 in that block,
    whose last record is taken behind the row.  A wrong bit in an earlier block
    moves the same counts and more records.  (Six ranges: the lanes of three
    and of one are the same lanes.)"""
    cat_off, _, matched, ignored, num_gt = _every_word_case(seed, junk, 6)[:5]
    for k in range(len(EVERY_SIZES)):
        a, b = int(cat_off[k]), int(cat_off[k + 1])
        off = np.array([0, b - a], np.int32)
        m0, i0, ng = matched[a:b], ignored[a:b], num_gt[k:k + 1]
        base_p, base_r = _oracle(off, m0, i0, ng)
        first = (b - a - 1) // WAVE * WAVE           # the last block's first row
        tp = m0[:, 0] & ~i0[:, 0]
        for r in range(6):
            # a TP bit: a valid row's matched bit, flipped
            bit = U64(1) << U64(N_THR * r + (k + r) % N_THR)
            rows = np.flatnonzero((i0[first:, 0] & bit) == 0)
            assert len(rows), (k, r)
            m1 = m0.copy()
            m1[first + rows[-1], 0] ^= bit
            got_p, got_r = _oracle(off, m1, i0, ng)
            assert not np.array_equal(got_r, base_r), (k, r)
            # a valid bit: an unmatched row in front of the last TP of the lane
            # whose TP total is num_gt
            full = [t for t in range(N_THR)
                    if int(((tp >> U64(N_THR * r + t)) & U64(1)).sum()) == ng[0, r]]
            bit = U64(1) << U64(N_THR * r + full[0])
            last_tp = np.flatnonzero(tp[first:] & bit)
            rows = np.flatnonzero((m0[first:, 0] & bit) == 0)
            assert len(last_tp) and len(rows) and rows[0] < last_tp[-1], (k, r)
            i1 = i0.copy()
            i1[first + rows[0], 0] ^= bit
            got_p, got_r = _oracle(off, m0, i1, ng)
            assert np.array_equal(got_r, base_r), (k, r)
            assert not np.array_equal(got_p, base_p), (k, r)


@pytest.fixture(params=["lookback", "twopass"])
def onepass_mode(request):
    _lib.sweep_mode(request.param)
    yield request.param
    _lib.sweep_mode("auto")


@gpu
@pytest.mark.parametrize("n_rng", [6, 3, 1])
@pytest.mark.parametrize("seed,junk", EVERY_INPUTS)
def test_every_word_through_the_compact_sweep(onepass_mode, seed, junk, n_rng):
    """All 2^18 words once each (three permutations, and one with anything in
    bits 18-30): the compact sweep, prepared and not, against the same rows
    expanded on the host and swept by the 16-byte gathered instance, and against
    the oracle.  num_gt is the one array all three are given."""
    from test_gpu_sweep_by_order import _device_tables
    case = _every_word_case(seed, junk, n_rng)
    cat_off, _, matched, ignored, num_gt, order, _, want_p, want_r = case
    hint = int(max(EVERY_SIZES))
    ref_p, ref_r, flag = _device_tables(cat_off, matched, ignored, num_gt, order, "paired",
                                        hint, "plain")
    assert flag == 0
    assert np.array_equal(ref_r, want_r) and np.array_equal(ref_p, want_p)
    for prepared in (False, True):
        got_p, got_r, flag = _compact_tables(case, hint, prepared)
        what = (onepass_mode, seed, junk, n_rng, prepared)
        assert flag == 0, what
        assert np.array_equal(got_r, ref_r) and np.array_equal(got_r, want_r), what
        assert np.array_equal(got_p, ref_p) and np.array_equal(got_p, want_p), what


# ---------------------------------------------------------------------------
# the blocking edges
# ---------------------------------------------------------------------------
EDGE_SIZES = [1, 63, 64, 65, 191, 192, 193, 383, 384, 385, 511, 512, 513, 2047, 2048, 2049,
              SC + CHUNK - 1, SC + CHUNK + 1, 2 * SC, 0, 3 * CHUNK + 200]
EDGE_PATTERNS = ["none"] + ["block%d" % b for b in range(8)] + \
    ["first_and_last", "whole_block", "whole_chunk"]


def _edge_escapes(pattern, sizes):
    """Sorted places whose rows are escaped.  blockB: one row of block B of
    every chunk that has one; first_and_last: the first and the last row of one
    block a chunk (block c % 8 of chunk c, where it exists, else the last
    one); whole_block: that block, whole; whole_chunk: every row of every
    second chunk, and of a category's only chunk."""
    esc = np.zeros(int(sum(sizes)), bool)
    rng = np.random.default_rng(43)
    at = 0
    for sz in sizes:
        for c, c0 in enumerate(range(0, sz, CHUNK)):
            c1 = min(c0 + CHUNK, sz)
            nblk = (c1 - c0 + WAVE - 1) // WAVE
            if pattern.startswith("block"):
                b = int(pattern[5:])
                if b < nblk:
                    b0, b1 = c0 + b * WAVE, min(c0 + (b + 1) * WAVE, c1)
                    esc[at + b0 + int(rng.integers(0, b1 - b0))] = True
            elif pattern in ("first_and_last", "whole_block"):
                b = min(c % 8, nblk - 1)
                b0, b1 = c0 + b * WAVE, min(c0 + (b + 1) * WAVE, c1)
                if pattern == "whole_block":
                    esc[at + b0:at + b1] = True
                else:
                    esc[at + b0] = esc[at + b1 - 1] = True
            elif pattern == "whole_chunk" and (c % 2 == 1 or sz <= CHUNK):
                esc[at + c0:at + c1] = True
        at += sz
    return esc


@functools.lru_cache(maxsize=None)
def _edge_case(pattern):
    """As test_gpu_compact_rows._sweep_case, on EDGE_SIZES: words in sorted order
    with anything in bits 18-30, rows = their expansion; an escaped place holds
    a row no word can say and a word that would expand to something else."""
    rng = np.random.default_rng(9)
    sizes = EDGE_SIZES
    K, n = len(sizes), int(sum(sizes))
    cat_off = np.zeros(K + 1, np.int32)
    np.cumsum(sizes, out=cat_off[1:])
    rank = np.concatenate([np.arange(s) / max(s, 1) for s in sizes])
    qpass = np.clip((rng.random(n) * 14 - 2 - 6 * rank).astype(np.int64), 0, 10)
    M = np.minimum(qpass, (rng.random(n) < 0.1) * rng.integers(0, 11, n))
    m10 = ((1 << qpass) - 1) & ~((1 << M) - 1)
    m10 = np.where(rng.random(n) < 0.1, rng.integers(0, 1024, n), m10)
    g = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 64, n))
    u = rng.random(n) < 0.15
    h = rng.random(n) < 0.05
    junk = rng.integers(0, 1 << 13, n)
    words = (m10 | g << 10 | u.astype(np.int64) << 16 | h.astype(np.int64) << 17 |
             junk << BITS).astype(np.uint32)
    m, i = expand_products(words)
    esc = _edge_escapes(pattern, sizes)
    ne = int(esc.sum())
    top = U64((1 << 60) - 1)
    m[esc] = rng.integers(0, 1 << 63, ne, dtype=np.uint64) & top
    i[esc] = rng.integers(0, 1 << 63, ne, dtype=np.uint64) & \
        rng.integers(0, 1 << 63, ne, dtype=np.uint64) & top
    words[esc] = ESCAPE | (rng.integers(0, 1 << 18, ne).astype(np.uint32) * (rng.random(ne) < 0.5))
    matched, ignored = m[:, None].copy(), i[:, None].copy()
    num_gt = np.zeros((K, 6), np.int32)
    for k in range(K):
        a, b = cat_off[k], cat_off[k + 1]
        for r in range(6):
            tp = int(((matched[a:b, 0] & ~ignored[a:b, 0]) >> U64(10 * r) & U64(1)).sum())
            num_gt[k, r] = 0 if (k + r) % 5 == 4 else \
                max(1, int(tp * (0.5 + rng.random())) + int(rng.integers(0, 3)))
    want_p, want_r = _oracle(cat_off, matched, ignored, num_gt)
    order = np.arange(n, dtype=np.int32)
    for a, b in zip(cat_off[:-1], cat_off[1:]):
        order[a:b] = a + rng.permutation(int(b - a))
    return cat_off, words, matched, ignored, num_gt, order, esc, want_p, want_r


def test_the_edge_patterns_put_escaped_rows_where_they_say():
    sizes = EDGE_SIZES
    assert {1, 63, 64, 65, 191, 192, 193, 383, 384, 385, 511, 512, 513, 2047, 2048, 2049,
            2048 + 512 - 1, 2048 + 512 + 1} <= set(sizes)
    k = sizes.index(2 * SC)
    assert sizes[k + 1] == 0          # ends on a super-chunk boundary, then an empty one
    at = int(sum(sizes[:k]))
    assert not _edge_escapes("none", sizes).any()
    for b in range(8):
        esc = _edge_escapes("block%d" % b, sizes)[at:at + 2 * SC].reshape(-1, 8, WAVE)
        assert (esc.sum(2) == np.eye(8, dtype=int)[b]).all()
    fl_ = _edge_escapes("first_and_last", sizes)[at:at + 2 * SC].reshape(-1, 8, WAVE)
    wb = _edge_escapes("whole_block", sizes)[at:at + 2 * SC].reshape(-1, 8, WAVE)
    for c in range(8):
        assert fl_[c].sum() == 2 and fl_[c, c, 0] and fl_[c, c, -1]
        assert wb[c].sum() == WAVE and wb[c, c].all()
    wc = _edge_escapes("whole_chunk", sizes)[at:at + 2 * SC].reshape(-1, CHUNK)
    assert wc.all(1).tolist() == [False, True] * 4 and (wc.all(1) == wc.any(1)).all()


@gpu
@pytest.mark.parametrize("pattern", EDGE_PATTERNS)
def test_plane_sweep_on_every_blocking_edge_with_escaped_rows(onepass_mode, pattern):
    """Category lengths on every edge of the blocking -- the block, the groups
    of three blocks (192, 384), the chunk, the super-chunk, one chunk beyond it
    -- and a category that ends on a super-chunk boundary in front of an empty
    one; escaped rows: none, one in each of a chunk's eight blocks in turn, the
    first and the last row of a block, a whole block, every row of a chunk."""
    case = _edge_case(pattern)
    esc, want_p, want_r = case[6:]
    assert bool(esc.any()) == (pattern != "none")
    for hint, prepared in ((0, False), (int(max(EDGE_SIZES)), False),
                           (int(max(EDGE_SIZES)), True)):
        got_p, got_r, flag = _compact_tables(case, hint, prepared)
        what = (onepass_mode, pattern, hint, prepared)
        assert flag == 0, what
        assert np.array_equal(got_r, want_r), what
        assert np.array_equal(got_p, want_p), what
