"""Box coordinates that are any double: the populations the box-value tests
share (test_box_values_host.py, test_gpu_box_values.py, test_gpu_edges.py,
golden/make_golden_maskapi.py) and the helpers that implant them into a
synth() or fixtures.rule_cells set.  A sibling of scorepop.py.

Both JSON readers take NaN / Infinity and exponents up to 1e308, and the
filters fence nothing in: a detection survives when 0 < w * h < inf (x, y
free, w and h may both be negative), a ground truth survives on its `area`
field (its bbox is entirely free).

box_population(kind, n, rng) returns n boxes [x, y, w, h] that come in PAIRS:
rows 2k and 2k + 1 are partners built to meet (row 2k is the side that a
detection takes, row 2k + 1 the side that a ground truth takes, which may
hold anything)."""
import numpy as np

from scorepop import DBL_MAX, NANS

KINDS = ("amodal", "touching", "flipped", "scales", "far", "nonfinite")
FINITE_KINDS = KINDS[:5]
FAR = 1e300                     # the task kernel's sentinel coordinate
FRAME_W, FRAME_H = 640.0, 480.0
TINY = 5e-324


def _decimal(rng, n, places):
    """n boxes around a 640 x 480 frame: inside, across an edge, negative x / y,
    wholly outside; coordinates with `places` decimals."""
    x = rng.uniform(-300.0, FRAME_W + 150.0, n)
    y = rng.uniform(-250.0, FRAME_H + 120.0, n)
    w = rng.uniform(0.5, 400.0, n)
    h = rng.uniform(0.5, 300.0, n)
    return np.round(np.stack([x, y, w, h], 1), places)


def _amodal(n_pairs, rng):
    a = np.where((rng.random(n_pairs) < 0.5)[:, None], _decimal(rng, n_pairs, 2),
                 _decimal(rng, n_pairs, 3))
    b = a.copy()                                    # a third: exact copies
    r = rng.random(n_pairs)
    near = (r >= 1 / 3) & (r < 2 / 3)               # a third: the copy moved and resized
    b[near, :2] += np.round(rng.uniform(-20, 20, (int(near.sum()), 2)), 2)
    b[near, 2:] = np.round(b[near, 2:] * rng.uniform(0.7, 1.3, (int(near.sum()), 2)), 2) + 0.01
    rest = r >= 2 / 3                               # a third: unrelated
    b[rest] = _decimal(rng, int(rest.sum()), 2)
    return a, b


def _touching(n_pairs, rng):
    a = _decimal(rng, n_pairs, 2)
    whole = rng.random(n_pairs) < 0.5
    a[whole] = np.rint(a[whole]) + np.array([0, 0, 1, 1.0])
    b = a.copy()
    x2, y2 = a[:, 0] + a[:, 2], a[:, 1] + a[:, 3]   # as the kernels round them
    for k in range(n_pairs):
        m = k % 7
        if m == 0:                                  # shared edge: width exactly 0
            b[k, 0] = x2[k]
        elif m == 1:                                # shared corner
            b[k, 0], b[k, 1] = x2[k], y2[k]
        elif m == 2:                                # nested
            b[k] = [a[k, 0] + a[k, 2] / 4, a[k, 1] + a[k, 3] / 4, a[k, 2] / 2, a[k, 3] / 2]
            if not whole[k]:
                b[k] = np.round(b[k], 3)
        elif m == 3:                                # one ulp short of touching (overlap)
            b[k, 0] = np.nextafter(x2[k], -np.inf)
        elif m == 4:                                # one ulp beyond touching
            b[k, 0] = np.nextafter(x2[k], np.inf)
        elif m == 5:                                # the same in y, from the other side
            b[k, 1] = np.nextafter(a[k, 1] - b[k, 3], rng.choice([-np.inf, np.inf]))
        else:                                       # edge shared from the left: b ends where a starts
            b[k, 0] = a[k, 0] - b[k, 2]
    return a, b


def _flipped(n_pairs, rng):
    """w < 0 and h < 0 together: the area is positive, the box passes both
    filters; x + w < x, so no rectangle ever meets it (IoU 0 by the formulas,
    never a negative width taken for an overlap)."""
    a, b = _amodal(n_pairs, rng)
    fa = rng.random(n_pairs) < 0.6
    a[fa, 2:] *= -1.0
    a[fa, :2] -= a[fa, 2:]                          # same corners, named from the other end
    fb = rng.random(n_pairs) < 0.4                  # some partners too, half of them in place
    b[fb, 2:] *= -1.0
    moved = fb & (rng.random(n_pairs) < 0.5)
    b[moved, :2] -= b[moved, 2:]
    return a, b


def _scales(n_pairs, rng):
    """Magnitudes 10 ** uniform(-160, 150), mixed within a pair; products that
    underflow to subnormal or zero; da + ga that overflows; w * h that is inf
    for finite w, h (a ground truth keeps such a box: it lives on `area`)."""
    def at(mag, m):
        u = rng.uniform(0.1, 1.0, (m, 4))
        u[:, :2] = rng.uniform(-1.0, 1.0, (m, 2))
        return u * mag[:, None]
    ma = 10.0 ** rng.uniform(-160, 150, n_pairs)
    a = at(ma, n_pairs)
    r = rng.random(n_pairs)
    mb = np.where(r < 0.5, ma, 10.0 ** rng.uniform(-160, 150, n_pairs))
    b = at(mb, n_pairs)
    same = np.flatnonzero(r < 0.5)
    b[same[::2], :2] = a[same[::2], :2]             # same corner: they do overlap
    for k in range(0, n_pairs, 4):                  # the named edges
        m = (k // 4) % 6
        if m == 0:      # intersection subnormal, areas subnormal
            a[k] = [0, 0, 3e-160, 2e-162]
            b[k] = [1e-160, 0, 3e-160, 2e-162]
        elif m == 1:    # intersection underflows to zero, areas do not
            a[k] = [0, 0, 1e-150, 1e-150]
            b[k] = [1e-150 - 1e-165, 1e-150 - 1e-165, 1e-150, 1e-150]
        elif m == 2:    # both areas finite, da + ga = inf: IoU exactly 0
            a[k] = [0, 0, 1.2e154, 1.2e154]
            b[k] = [1e153, 1e153, 1.2e154, 1.2e154]
        elif m == 3:    # ga = inf (finite w, h), da finite: i / inf = 0
            a[k] = [0, 0, 1e150, 1e149]
            b[k] = [0, 0, 1e160, 1e160]
        elif m == 4:    # both areas inf and the intersection too: inf - inf
            a[k] = [0, 0, 1e160, 1e150]
            b[k] = [1e100, 0, 1e160, 1e150]
        else:           # a large and a tiny box at one corner
            a[k] = [1e-150, 1e-150, 1e140, 1e140]
            b[k] = [1e-150, 1e-150, 1e-140, 1e-140]
    return a, b


FAR_X = np.array([FAR, np.nextafter(FAR, 0), np.nextafter(FAR, np.inf), 2e300, 1.5e300,
                  -FAR, -2e300, DBL_MAX, -DBL_MAX, 1e299])


def _far(n_pairs, rng):
    """Coordinates on, just below and above +-1e300 (x == 1e300 exactly), x + w
    and y + h above 1e300 with a finite area (w = 1e-100: the sum is x), +-
    DBL_MAX as x.  Six motifs in turn; a partner is a copy, a copy shifted by
    a quarter of the width (far boxes do intersect each other), or an ordinary
    box."""
    a = _decimal(rng, n_pairs, 2)
    beyond = np.array([2e300, 1.5e300, np.nextafter(FAR, np.inf)])
    big = 10.0 ** rng.uniform(285, 295, n_pairs)
    for k in range(n_pairs):
        m = k % 6
        if m == 0:          # x == 1e300 exactly, a real extent: meets its partner
            a[k, 0], a[k, 2] = FAR, big[k]
        elif m == 1:        # beyond 1e300 in both axes, x + w = x, finite area
            a[k] = [rng.choice(beyond), rng.choice(beyond), 1e-100, 1e-100]
        elif m == 2:        # any far x (either sign), x + w = x
            a[k, 0], a[k, 2] = rng.choice(FAR_X), 1e-100
        elif m == 3:        # +-DBL_MAX: x + w overflows on the positive side
            a[k, 0], a[k, 2] = rng.choice([DBL_MAX, -DBL_MAX]), rng.choice([1e293, 1e295])
        elif m == 4:        # area just below DBL_MAX: da + ga overflows
            a[k, 0], a[k, 2], a[k, 3] = rng.choice(FAR_X[:5]), 1e295, 1.2e13
        else:               # around 1e300 in x, at it in y, no height left
            a[k] = [rng.choice(FAR_X[:3]), FAR, big[k], 1e-100]
    b = a.copy()
    r = rng.random(n_pairs)
    move = r < 0.4
    with np.errstate(over="ignore"):               # (DBL_MAX + w / 4 = inf: that partner stays a copy)
        moved = b[:, 0] + 0.25 * b[:, 2]
    move &= np.isfinite(moved)
    b[move, 0] = moved[move]
    b[r > 0.8] = _decimal(rng, int((r > 0.8).sum()), 2)
    return a, b


NONFINITE = np.concatenate([NANS, [np.inf, -np.inf]])


def _nonfinite(n_pairs, rng):
    """Row 2k (a detection's side): NaN in three bit patterns and +-inf in x
    and y, -0.0 and +-5e-324 anywhere; w, h stay ordinary, so the box
    survives 0 < w * h < inf.  Row 2k + 1 (a ground truth's side): the same
    values in ANY member."""
    a, b = _amodal(n_pairs, rng)
    for k in range(n_pairs):
        m = k % 8
        v = NONFINITE[rng.integers(0, len(NONFINITE))]
        if m == 0:
            a[k, 0] = v
        elif m == 1:
            a[k, 1] = v
        elif m == 2:
            a[k, 0], a[k, 1] = v, NONFINITE[rng.integers(0, len(NONFINITE))]
        elif m == 3:
            a[k, rng.integers(0, 2)] = rng.choice([-0.0, TINY, -TINY])
        elif m == 4:                                # inf against the same inf: inf - inf
            a[k, 0] = b[k, 0] = rng.choice([np.inf, -np.inf])
        elif m == 5:
            a[k, rng.integers(0, 4)] = rng.choice([-0.0, TINY, -TINY])
        w = rng.integers(0, 4)
        if k % 3 != 2:
            b[k, w] = NONFINITE[rng.integers(0, len(NONFINITE))]
        elif k % 2:
            b[k, w] = rng.choice([-0.0, TINY, -TINY])
    return a, b


_MAKERS = dict(amodal=_amodal, touching=_touching, flipped=_flipped, scales=_scales,
               far=_far, nonfinite=_nonfinite)


def box_population(kind, n, rng):
    """n boxes [x, y, w, h] of one of KINDS; rows 2k, 2k + 1 are partners."""
    n_pairs = (n + 1) // 2
    a, b = _MAKERS[kind](n_pairs, rng)
    out = np.empty((2 * n_pairs, 4))
    out[0::2], out[1::2] = a, b
    return np.ascontiguousarray(out[:n])


def survives(box):
    """The detection filter: 0 < w * h < inf."""
    with np.errstate(all="ignore"):
        area = box[:, 2] * box[:, 3]
    return (area > 0) & (area < np.inf)


def golden_boxes(kind):
    """(dt[256, 4], gt[96, 4]) of the bbIou golden (maskapi/bb_iou_domain.npz):
    dt row k and gt row k are partners for k < 96."""
    pop = box_population(kind, 512, np.random.default_rng([0xb0c5, KINDS.index(kind)]))
    return np.ascontiguousarray(pop[0::2]), np.ascontiguousarray(pop[1::2][:96])


# ---------------------------------------------------------------------------
# implanting a population into a set
# ---------------------------------------------------------------------------
def implant(gt, dt, kind, rng, gt_share=0.25, dt_share=0.1):
    """Give a share of gt.ann_bbox and of dt.bbox boxes of `kind`, in place
    (new arrays: the columns are not written through).  A changed ground truth
    takes row 2k + 1 of the population; up to two detections of its image and
    category take row 2k, the partner, so that the pairs meet in a cell.  A
    further `dt_share` of the detections takes detection-side boxes on their
    own.  ann_area stays as it was: the ground truths stay evaluated.  Returns
    (changed ground-truth rows, changed detection rows); at least half of the
    changed detections survive 0 < w * h < inf."""
    g_rows = np.flatnonzero(rng.random(len(gt.ann_id)) < gt_share)
    pop = box_population(kind, 2 * max(len(g_rows), 1), rng)
    gbox, dbox = np.array(gt.ann_bbox, dtype=np.float64), np.array(dt.bbox, dtype=np.float64)
    key = lambda img, cat: img.astype(np.int64) * (1 << 20) + cat    # noqa: E731
    dkey = key(np.asarray(dt.image_id), np.asarray(dt.category_id))
    order = np.argsort(dkey, kind="stable")
    skey = dkey[order]
    gkey = key(np.asarray(gt.ann_img), np.asarray(gt.ann_cat))
    taken = np.zeros(len(dbox), bool)
    for j, g in enumerate(g_rows):
        gbox[g] = pop[2 * j + 1]
        lo, hi = np.searchsorted(skey, gkey[g]), np.searchsorted(skey, gkey[g], "right")
        free = [r for r in order[lo:hi] if not taken[r]][:2]
        for r in free:
            dbox[r] = pop[2 * j]
            taken[r] = True
    extra = np.flatnonzero((rng.random(len(dbox)) < dt_share) & ~taken)
    dbox[extra] = box_population(kind, 2 * max(len(extra), 1), rng)[0::2][:len(extra)]
    taken[extra] = True
    d_rows = np.flatnonzero(taken)
    assert len(d_rows) and survives(dbox[d_rows]).mean() >= 0.5, kind
    gt.ann_bbox, dt.bbox = gbox, dbox
    return g_rows, d_rows
