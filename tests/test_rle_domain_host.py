"""The run-length population of tests/rlepop.py on the host: the oracle
(oracle/rle.py, tests/track_segm_ref.py) against the recording of the reference
C on the same pairs (golden/maskapi/rle_domain.npz), the stop rule against the
oracle, the population against its own claims, and what the host library
refuses."""
import numpy as np
import pytest

import rlepop
import track_segm_ref as ref
from goldenio import path
from oracle import rle
from tao_amodal_amd.masks import MaskBatch


@pytest.fixture(scope="module")
def golden():
    return np.load(path("maskapi", "rle_domain.npz"))


@pytest.mark.parametrize("kind", rlepop.PAIR_KINDS)
def test_oracle_equals_the_reference_c_on_every_pair(kind, golden):
    pairs = rlepop.pairs_of(kind)[0]
    iou, inter, union = (golden[kind + s] for s in ("_iou", "_inter", "_union"))
    assert len(iou) == len(inter) == len(union) == len(pairs)
    for k, (d, g) in enumerate(pairs):
        assert rle.iou_pair(d, g) == iou[k], (kind, k)
        assert ref.frame_terms(d, g) == (int(inter[k]), int(union[k])), (kind, k)


@pytest.mark.parametrize("kind", rlepop.PAIR_KINDS)
def test_stop_rule_predicts_the_oracle(kind):
    for k, (d, g) in enumerate(rlepop.pairs_of(kind)[0]):
        i, u = rlepop.predicted(d, g)
        assert ref.frame_terms(d, g) == (i, u), (kind, k)
        if rle.bb_overlap(rle.to_bbox(d), rle.to_bbox(g)):
            assert rle.iou_pair(d, g) == (i / u if i else 0.0), (kind, k)


def test_stop_rule_on_random_pairs_with_empty_runs():
    rng = np.random.default_rng(77)
    stopped = 0
    for _ in range(400):
        n = int(rng.integers(4, 40))
        ends = np.sort(rng.integers(0, n + 1, size=(2, int(rng.integers(1, 12)))), axis=1)
        a, b = (rlepop.from_ends(n, e, lead=bool(rng.integers(2))) for e in ends)
        d, g = rlepop.mask(1, n, a), rlepop.mask(1, n, b)
        assert ref.frame_terms(d, g) == rlepop.predicted(d, g), (a, b)
        stopped += rlepop.stop_pixel(a, b) < n
    assert stopped > 40


def test_the_table_rows_of_the_stop_rule():
    want = [(0.0, (0, 0)), (1.0, (4, 4)), (0.0, (0, 2))]
    for (a, b), (iou, terms) in zip(rlepop.TABLE_ROWS, want):
        d, g = rlepop.mask(2, 3, a), rlepop.mask(2, 3, b)
        assert rle.iou_pair(d, g) == iou and ref.frame_terms(d, g) == terms
    # with every pixel counted the first row would give 4 / 4, and the third
    # a union of 5, not 2
    assert rlepop.count_before(*rlepop.TABLE_ROWS[0], 6) == (4, 4)
    assert rlepop.count_before(*rlepop.TABLE_ROWS[2], 6) == (0, 5)


# ------------------------------------------------------- the population's claims
def _ends(c):
    return np.cumsum(c, dtype=np.int64)


def test_pieces_claims():
    pairs, c = rlepop.pieces()
    ka = [len(d["counts"]) for d, _ in pairs]
    kb = [len(g["counts"]) for _, g in pairs]
    assert set(ka) == set(rlepop.KA) == c["ka"] and set(kb) == set(rlepop.KB) == c["kb"]
    assert sum(k > rlepop.PIECE for k in ka) == c["multi_piece"] >= 20
    for k in rlepop.KA:          # a short, a middling and a long partner each
        mine = sorted(b for a, b in zip(ka, kb) if a == k)
        assert mine[0] <= 9 and 63 <= mine[len(mine) // 2] <= 129 and mine[-1] >= 1023, k
    for k in rlepop.KB:
        mine = sorted(a for a, b in zip(ka, kb) if b == k)
        assert mine[0] <= 9 and mine[-1] >= 1023 and any(15 <= a <= 513 for a in mine), k
    for parity in (0, 1):        # the last run of ones / of zeros, with and without a lead
        for lead in (False, True):
            assert any(len(d["counts"]) % 2 == parity and (d["counts"][0] == 0) == lead
                       and len(d["counts"]) > rlepop.PIECE for d, _ in pairs)
    assert c["lead_a"] > 30 and c["lead_b"] > 30
    assert not any(rlepop.has_empty(m["counts"]) and len(m["counts"]) > 2
                   for p in pairs for m in p)
    assert all(rlepop.stop_pixel(d["counts"], g["counts"]) == rlepop.N for d, g in pairs)


def test_dense_claims():
    pairs, c = rlepop.dense()
    between = [rlepop.most_between(d["counts"], g["counts"]) for d, g in pairs]
    assert sum(b > rlepop.FOLLOW for b in between) >= c["bisect"]
    assert sum(b >= 1990 for b in between) >= 8                # thousands inside one run
    # B's stretch ends 0..5 runs behind a boundary of A
    tails = set()
    for d, g in pairs[:24:2]:
        ea, eb = _ends(d["counts"]), _ends(g["counts"])
        x = ea[-3]
        tails.add(int(((eb > x) & (eb <= ea[-2])).sum()))
    assert tails == {0, 1, 2, 3, 4, 5}
    assert sum(len(d["counts"]) % 2 == 0 and len(g["counts"]) > 1000 for d, g in pairs) >= 3
    assert sum(len(d["counts"]) > 2000 and len(g["counts"]) <= 5 for d, g in pairs) == 12


def test_ties_claims():
    pairs, c = rlepop.ties()
    shared = [len(np.intersect1d(_ends(d["counts"])[:-1], _ends(g["counts"])[:-1]))
              for d, g in pairs]
    assert sum(s >= 10 for s in shared) >= 24
    ious = [rle.iou_pair(d, g) for d, g in pairs]
    assert sum(v == 1.0 for v in ious) == c["identical"]
    assert sum(v == 0.0 for v in ious) == c["complements"]
    assert all(rlepop.stop_pixel(d["counts"], g["counts"]) == rlepop.N for d, g in pairs)


def test_empty_runs_claims():
    pairs, c = rlepop.empty_runs()
    got = [rlepop.stop_pixel(d["counts"], g["counts"]) for d, g in pairs]
    want = [m["h"] * m["w"] if p is None else p for (m, _), p in zip(pairs, c["stop_at"])]
    assert got == want and c["stopped"] == 12
    assert 0 in want                                            # a stop at pixel 0
    flagged = [(rlepop.has_empty(d["counts"]), rlepop.has_empty(g["counts"])) for d, g in pairs]
    unstopped = {f for f, p in zip(flagged, c["stop_at"]) if p is None}
    assert {(True, False), (False, True), (True, True)} <= unstopped
    beyond = [(d, g, p) for (d, g), p in zip(pairs, c["stop_at"]) if p is not None
              and np.searchsorted(_ends(d["counts"]), p) > rlepop.PIECE]
    assert len(beyond) == 1                                     # a stop in A's second piece
    zero = [(d, g) for (d, g), p in zip(pairs, c["stop_at"])
            if p is not None and p > 3 and ref.frame_terms(d, g)[0] == 0]
    assert len(zero) >= 2 and all(ref.frame_terms(d, g)[1] > 1 and rle.iou_pair(d, g) == 0.0
                                  for d, g in zero)
    assert [(d["counts"], g["counts"]) for d, g in pairs[-3:]] == \
        [(list(a), list(b)) for a, b in rlepop.TABLE_ROWS]


def test_big_frames_claims():
    pairs, c = rlepop.big_frames()
    assert c["frames"] == [(1 << 31) - 1, 1 << 31, (1 << 32) - 1, (1 << 31) + 6]
    assert {d["h"] * d["w"] for d, _ in pairs} == set(c["frames"])
    assert len(pairs) == rlepop.PER_BIG * len(c["frames"])
    # what passes 2^31 and 2^32 among the pairs that go through the prefix sums
    fast = [(d, g) for d, g in pairs if not rlepop.literal(d, g)]
    terms = [ref.frame_terms(d, g) for d, g in fast]
    assert 25 <= len(fast) < len(pairs)
    assert sum(i >= rlepop.TWO31 for i, _ in terms) >= 3
    assert sum(u >= rlepop.TWO31 for _, u in terms) >= 12
    assert sum(rle.area(d) + rle.area(g) >= rlepop.TWO32 for d, g in fast) >= 3
    assert sum(len(d["counts"]) > rlepop.PIECE for d, _ in fast) >= 8
    # the two current runs hold 2^32 pixels between them: the reference stops
    wrapped = [k for k, (d, g) in enumerate(pairs)
               if rlepop.stop_pixel(d["counts"], g["counts"]) < d["h"] * d["w"]]
    assert len(wrapped) == 5 and all(rlepop.literal(*pairs[k]) for k in wrapped)
    assert all(not rlepop.has_empty(m["counts"][1:]) for k in wrapped for m in pairs[k])


def test_cells_claims():
    cells, c = rlepop.cells()
    assert {1, 63, 64, 65, 128, 129} <= c["G"] and {1, 7, 8, 9, 17} <= c["D"]
    assert {0, 63, 64, 128} <= c["walked_lanes"]
    assert {6143, 6144, 6145} <= c["gt_runs"] and max(c["gt_runs"]) == 6145
    assert cells[-1] == ([], [])
    assert any(not d and g for d, g in cells[:-1]) and any(d and not g for d, g in cells[:-1])
    kinds = set()                # a tile with holes: 0, -1 and walked pairs side by side
    for dts, gts in cells:
        if len(gts) >= 63:
            row = rle.iou_matrix(dts[:1], gts)[0]
            walked = np.array([any(g["h"] == d["h"] and
                                   rle.bb_overlap(rle.to_bbox(d), rle.to_bbox(g)) for d in dts)
                               for g in gts])
            kinds.add((bool((row == 0).any()), bool((row == -1).any()), bool(walked.any())))
            assert walked[0] and walked[63:65].all() and not walked.all()
    assert kinds == {(True, True, True)}
    late_stop = [1 for dts, gts in cells for j, g in enumerate(gts) if j >= 64 for d in dts
                 if d["h"] == g["h"] and d["w"] == g["w"] and sum(d["counts"]) == sum(g["counts"])
                 and rlepop.stop_pixel(d["counts"], g["counts"]) < sum(g["counts"])]
    assert len(late_stop) >= 1


def test_tracks_claims():
    probs, c = rlepop.tracks()
    assert c["pairs"] == [3, 4, 5] and {63, 64, 65, 129} <= c["dt_frames"]
    shared = sorted(ref.shared_frames(d, g) for p in probs for dts, gts in p
                    for d in dts for g in gts)
    assert shared[0] == 0 and shared[-1] == 129 and 2 in shared
    assert any(not gts and dts for dts, gts in probs[2][:-2])   # G = 0 before the last cell
    pool = rlepop.frame_pool()
    stops = sum(rlepop.stop_pixel(d["counts"], g["counts"]) < sum(d["counts"]) for d, g in pool)
    assert stops >= 12 and sum(d["h"] * d["w"] >= rlepop.TWO31 - 1 for d, _ in pool) >= 12
    pairs, share = rlepop.column_edges()
    for (d, g), s in zip(pairs, share):          # h = 1: a pixel is a column
        assert ref.frame_terms(d, g)[0] == s
    assert {(len(d["counts"]) & 1, len(g["counts"]) & 1, s) for (d, g), s in zip(pairs, share)} >= \
        {(1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (0, 0, 1)}


# ------------------------------------------------------------ outside the domain
def test_run_lists_of_2_to_32_pixels_or_more_are_refused():
    b = MaskBatch()
    top = (1 << 32) - 1
    ok = b.add({"size": [65535, 65537], "counts": [0, top]}, 0, 0)
    assert b.add({"size": [65535, 65537], "counts": rle.to_string({"counts": [7, top - 7]})}, 0, 0) \
        == ok + 1
    for counts in ([1, top], [1 << 31, 1 << 31], [top, 0, top]):
        with pytest.raises(ValueError):
            b.add({"size": [65536, 65536], "counts": counts}, 0, 0)
        with pytest.raises(ValueError):
            b.add({"size": [65536, 65536], "counts": rle.to_string({"counts": counts})}, 0, 0)
    for size in ([1 << 31, 1], [1, 1 << 31]):
        with pytest.raises(ValueError):
            b.add({"size": size, "counts": [5]}, 0, 0)
        with pytest.raises(ValueError):
            b.add({"size": size, "counts": rle.to_string({"counts": [5]})}, 0, 0)
    assert len(b) == 2                               # a refused mask leaves nothing behind
    a = b.arrays()
    assert a.mask(0)["counts"] == [0, top] and a.mask(1)["counts"] == [7, top - 7]
    b.close()
