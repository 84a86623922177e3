"""Box coordinates that are any double, on the host (no GPU): the C oracle
and oracle/pyoracle.py against the reference's compiled bbIou on the
populations of tests/boxpop.py (its answers stored as
golden/maskapi/bb_iou_domain.npz), and the C oracle's track IoU against the
reference's Python statement.

Contract ("Box coordinates: the domain"): the image level equals
the reference's compiled bbIou everywhere; the track level equals the
reference's Python on every finite input, returns i / u where the reference's
``assert i <= u`` would fire, and on non-finite input follows C's fmin / fmax
and ``w > 0 ? w : 0`` where Python's max / min depend on the operand order."""
import types

import numpy as np
import pytest

import boxpop
import orclib
from boxpop import KINDS
from goldenio import path
from oracle import pyoracle
from scorepop import same_values

MODES = ("3d_iou", "avg_iou", "imagenetvid")


@pytest.fixture(scope="module")
def golden():
    return np.load(path("maskapi", "bb_iou_domain.npz"))


@pytest.mark.parametrize("kind", KINDS)
def test_golden_boxes_are_the_population(golden, kind):
    """The stored boxes are what boxpop.golden_boxes draws today, as bits."""
    dt, gt = boxpop.golden_boxes(kind)
    assert np.array_equal(dt.view(np.uint64), golden[kind + "_dt"].view(np.uint64))
    assert np.array_equal(gt.view(np.uint64), golden[kind + "_gt"].view(np.uint64))
    assert golden[kind + "_iou"].shape == (256, 96)
    assert np.isfinite(dt).all() and np.isfinite(gt).all() or kind == "nonfinite"
    assert boxpop.survives(dt).mean() >= 0.5


@pytest.mark.parametrize("kind", KINDS)
def test_c_oracle_bb_iou_equals_the_reference_build(golden, kind):
    """NaN where the golden has NaN, bit-equal elsewhere."""
    got = orclib.bb_iou(golden[kind + "_dt"], golden[kind + "_gt"])
    assert same_values(got, golden[kind + "_iou"])


@pytest.mark.reference
@pytest.mark.parametrize("kind", KINDS)
def test_golden_equals_the_live_reference_build(golden, kind):
    got = orclib.ref_bb_iou(golden[kind + "_dt"], golden[kind + "_gt"])
    assert same_values(got, golden[kind + "_iou"])
    assert same_values(got, orclib.bb_iou(golden[kind + "_dt"], golden[kind + "_gt"]))


def crowd_column(kind, n=96):
    """The iscrowd column the crowd tests use: about a third of the ground truths."""
    return (np.random.default_rng([0xc0, KINDS.index(kind)]).random(n) < 0.35).astype(np.uint8)


@pytest.mark.reference
@pytest.mark.parametrize("kind", KINDS)
def test_c_oracle_bb_iou_with_crowd_equals_the_live_reference_build(golden, kind):
    """The C oracle's iscrowd branch (what taoamd_bb_iou is compared with on
    the device) against the reference's own."""
    dt, gt, crowd = golden[kind + "_dt"], golden[kind + "_gt"], crowd_column(kind)
    assert 10 < crowd.sum() < 86
    assert same_values(orclib.bb_iou(dt, gt, crowd), orclib.ref_bb_iou(dt, gt, crowd))


@pytest.mark.parametrize("kind", KINDS)
def test_pyoracle_bb_iou_equals_the_reference_build(golden, kind):
    """The Python restatement with C's fmin / fmax (Python's min / max return
    an operand that depends on the order when one is NaN: [nan, 0, 10, 10]
    against [0, 0, 10, 10] gave nan where bbIou gives 1.0)."""
    dt, gt = golden[kind + "_dt"].tolist(), golden[kind + "_gt"].tolist()
    got = np.array([[pyoracle.bb_iou(d, g) for g in gt] for d in dt])
    assert same_values(got, golden[kind + "_iou"])
    assert pyoracle.bb_iou([float("nan"), 0, 10, 10], [0, 0, 10, 10]) == 1.0


@pytest.mark.parametrize("kind", ["scales", "far", "nonfinite"])
def test_golden_holds_the_edges(golden, kind):
    """From the reference's answers alone: NaN IoUs, IoUs that are exactly 0
    through an infinite union, and finite positive ones."""
    dt, gt, iou = golden[kind + "_dt"], golden[kind + "_gt"], golden[kind + "_iou"]
    with np.errstate(all="ignore"):
        union = (dt[:, 2] * dt[:, 3])[:, None] + (gt[:, 2] * gt[:, 3])[None, :]
    assert np.isnan(iou).sum() >= 20
    assert ((iou == 0) & np.isinf(union)).sum() >= 20
    assert (np.isfinite(iou) & (iou > 0)).sum() >= 20


def test_golden_amodal_copies_reach_one_and_above(golden):
    """Exact copies: IoU 1, or above 1 by the rounding of (x + w) - x."""
    iou = golden["amodal_iou"]
    assert (iou == 1).sum() >= 10 and (iou > 1).sum() >= 3


# ---------------------------------------------------------------------------
# track level: the C oracle against the reference's Python statement
# ---------------------------------------------------------------------------
def _track_pairs(kind, n_pairs, seed):
    """n_pairs (detection track, ground-truth track) pairs of 1 to 20 timeline
    positions, each side with holes (a position holds a detection box, a
    ground-truth box, both -- partners of the population -- or, inside a longer
    track, neither); returns the per-pair lists [(pos, box)]."""
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    out = []
    for _ in range(n_pairs):
        n = int(rng.integers(1, 21))
        pop = boxpop.box_population(kind, 2 * n, rng)
        has_d, has_g = rng.random(n) < 0.7, rng.random(n) < 0.7
        has_d[rng.integers(0, n)] = True
        has_g[rng.integers(0, n)] = True
        out.append(([(p, pop[2 * p]) for p in range(n) if has_d[p]],
                    [(p, pop[2 * p + 1]) for p in range(n) if has_g[p]]))
    return out


def _as_tables(pairs):
    """One cell per pair, for orclib.track_iou."""
    f = types.SimpleNamespace()
    n = len(pairs)
    f.n_cells = n
    f.cell_dt_off = np.arange(n + 1, dtype=np.int32)
    f.cell_gt_off = np.arange(n + 1, dtype=np.int32)
    f.cell_iou_off = np.arange(n + 1, dtype=np.int64)
    for side, k in (("dt", 0), ("gt", 1)):
        lens = [len(p[k]) for p in pairs]
        setattr(f, side + "_frame_off", np.r_[0, np.cumsum(lens)].astype(np.int32))
        setattr(f, side + "_frame_pos",
                np.array([q for p in pairs for q, _ in p[k]], dtype=np.int32))
        setattr(f, side + "_frame_box",
                np.array([b for p in pairs for _, b in p[k]], dtype=np.float64).reshape(-1, 4))
    return f


def _python_statement(pairs, mode, fired=None):
    """pyoracle's functions (the reference's text) in timeline order."""
    out = []
    for dts, gts in pairs:
        dmap = {p: b.tolist() for p, b in dts}
        gmap = {p: b.tolist() for p, b in gts}
        timeline = {p: p for p in set(dmap) | set(gmap)}
        if mode == "3d_iou":
            log = []
            out.append(pyoracle.track_box_iou(dmap, gmap, "timeline", timeline, log))
            if fired is not None:
                fired.append(bool(log))
        elif mode == "avg_iou":
            out.append(pyoracle.track_avg_iou(dmap, gmap, "timeline", timeline))
        else:
            out.append(pyoracle.track_imagenetvid_iou(dmap, gmap))
    return np.array(out, dtype=np.float64)


@pytest.mark.parametrize("kind", boxpop.FINITE_KINDS)
def test_c_oracle_track_iou_equals_the_reference_statement_on_finite_boxes(kind):
    """Bit for bit in all three modes, with the assert switched to reporting."""
    pairs = _track_pairs(kind, 300, 11)
    f = _as_tables(pairs)
    for mode in MODES:
        got, _ = orclib.track_iou(f, mode)
        want = _python_statement(pairs, mode)
        assert same_values(got, want), (kind, mode, np.flatnonzero(
            ~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])


# what the counting test below measured; DESIGN.md quotes the two numbers
NONFINITE_PAIRS = 600
NONFINITE_DIFFER = {"3d_iou": 25, "avg_iou": 238, "imagenetvid": 282}
NONFINITE_WOULD_RAISE = 589


def test_nonfinite_track_iou_differs_by_the_two_named_rules_only():
    """On non-finite boxes the C oracle (the contract) leaves the reference's
    Python: max(nan, g) is nan in Python while fmax is g, and max(nan, 0) is
    nan while ``w > 0 ? w : 0`` is 0.  With exactly these two rules put into
    the statement the two agree bit for bit; the counts of pairs that differ
    without them, and of pairs on which the reference dies on its assert, are
    pinned."""
    pairs = _track_pairs("nonfinite", NONFINITE_PAIRS, 12)
    f = _as_tables(pairs)
    fired = []
    differ = {}
    for mode in MODES:
        got, _ = orclib.track_iou(f, mode)
        py = _python_statement(pairs, mode, fired if mode == "3d_iou" else None)
        differ[mode] = int((~((got == py) | (np.isnan(got) & np.isnan(py)))).sum())
        keep = pyoracle.bb_intersect_union
        pyoracle.bb_intersect_union = pyoracle.bb_intersect_union_c
        try:
            want = _python_statement(pairs, mode)
        finally:
            pyoracle.bb_intersect_union = keep
        assert same_values(got, want), mode
    print("nonfinite: differ", differ, "would raise", sum(fired), "of", len(pairs))
    assert differ == NONFINITE_DIFFER
    assert sum(fired) == NONFINITE_WOULD_RAISE


def test_identical_decimal_tracks_give_i_over_u_where_the_reference_asserts():
    """A one-frame track that copies its ground truth: (x + w) - x > w by
    rounding for about a third of 2- and 3-decimal boxes, so i > u and the
    reference's ``assert i <= u`` fires on ordinary input.  The C oracle (and
    the product) return i / u, just above 1."""
    rng = np.random.default_rng(13)
    a, b = boxpop._amodal(4000, rng)
    same = np.flatnonzero((a == b).all(axis=1))[:1000]
    assert len(same) == 1000
    pairs = [([(0, a[k])], [(0, b[k])]) for k in same]
    fired = []
    want = _python_statement(pairs, "3d_iou", fired)
    assert sum(fired) >= 100, sum(fired)
    got, _ = orclib.track_iou(_as_tables(pairs), "3d_iou")
    iu = [pyoracle.bb_intersect_union(d[0][1].tolist(), g[0][1].tolist()) for d, g in pairs]
    assert np.array_equal(got, np.array([i / u for i, u in iu]))
    assert np.array_equal(got, want)
    hit = np.array(fired)
    assert (got[hit] > 1).all() and (got[~hit] <= 1).all()
    with pytest.raises(AssertionError):
        k = int(np.flatnonzero(hit)[0])
        d, g = pairs[k]
        pyoracle.track_box_iou({0: d[0][1].tolist()}, {0: g[0][1].tolist()}, "timeline", {0: 0})
    # the issue's example
    assert pyoracle.bb_intersect_union([0.1, 0.1, 0.2, 0.2], [0.1, 0.1, 0.2, 0.2]) == \
        (0.040000000000000015, 0.04)
