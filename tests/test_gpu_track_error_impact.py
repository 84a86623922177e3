"""-m gpu: the track-level error impact (taoamd_track_error_types_links,
taoamd_track_error_impact, engine.stage_track_error_impact,
TaoEval.error_impact) against the numpy restatement of
tests/track_error_impact_ref.py.  The restatement's IoUs are the C oracle's, the
kernels' arithmetic in the kernels' order, the links are indices and the sweep
is the reference's own expression: every comparison is exact."""
import numpy as np
import pytest

import boxpop
import error_impact_ref as imp_ref
import orclib
import test_gpu_error_impact as img
import test_gpu_track_error_types as trk
import track_error_impact_ref as ref
import track_error_types_ref as te
import wsguard
from tao_amodal_amd import _lib
from test_gpu_error_impact import _same, _same_links, bare_tables
from test_gpu_track_error_types import _csr, _device_match, _frames, _seeded_table, _up

from constants_cases import cases, edit     # (tests/golden: on the path since trk's import)

pytestmark = pytest.mark.gpu

N_THR, N_REC = _lib.N_THR, _lib.N_REC
TILE = _lib.TRACK_ERROR_TYPES_TILE     # TE_G: ground-truth tracks per LDS tile
LANES = 256                            # TE_LANES: detection tracks per round of a video
CHUNK_POS = 8                          # TE_P: timeline positions per staged chunk
DEV = "cuda:0"
NAN = float("nan")
SETTINGS = ((0, 0.1), (5, 0.25), (0, 0.0))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _device_links(f, iou, mg, gt_rng, dt_rng, n_rng, slot, tb, status=False, ws_bytes=None,
                  lists=None, drop=None):
    """taoamd_track_error_types_links on a Flat; the workspace is exactly the
    size taoamd_track_error_types_workspace reports, behind a guard band.
    `lists`: (vid_gt_off, vid_gt, vid_dt_off, vid_dt) instead of the table's
    own; `drop`: which of the three tables to leave out."""
    import torch
    lib = _lib.load()
    n_dt, n_gt = int(f.cell_dt_off[-1]), int(f.cell_gt_off[-1])
    n_vid, K = len(f.vid_ids), len(f.cat_ids)
    d_vid, g_vid = te.units(f)
    if lists is None:
        lists = _csr(g_vid, n_vid) + _csr(d_vid, n_vid)
    lists = [_up(x, np.int32) for x in lists]
    d_off, g_off = np.asarray(f.cell_dt_off), np.asarray(f.cell_gt_off)
    d_cell = np.repeat(np.arange(f.n_cells), np.diff(d_off))
    group = np.stack([g_off[d_cell], np.diff(g_off)[d_cell], np.arange(n_dt) - d_off[d_cell],
                      d_cell], 1) if n_dt else np.zeros((0, 4))
    cols = [_up(f.dt_cat, np.int32), _up(dt_rng, np.uint32).view(torch.int32),
            _up(group, np.int32), _up(f.cell_iou_off, np.int64), _up(iou, np.float64),
            _up(mg, np.int32)]
    gcols = [_up(f.gt_cat, np.int32), _up(gt_rng, np.uint32).view(torch.int32)]
    fr = _frames(f)
    rows, width = max(n_dt, 1), max(n_rng, 1)
    dt_counts = torch.full((width, K, 7), -3, dtype=torch.int64, device=DEV)
    gt_counts = torch.full((width, K, 3), -3, dtype=torch.int64, device=DEV)
    dt_type = torch.full((rows, width), 99, dtype=torch.uint8, device=DEV)
    dt_over = torch.full((rows, 2), -1, dtype=torch.int32, device=DEV)
    same = torch.full((rows, width), -9, dtype=torch.int32, device=DEV)
    other = torch.full((rows, width), -9, dtype=torch.int32, device=DEV)
    held = torch.full((width, max(n_gt, 1)), 7, dtype=torch.uint8, device=DEV)
    need = lib.taoamd_track_error_types_workspace(n_dt, n_gt, min(max(n_rng, 1), 20))
    ws = wsguard.Guarded(need if ws_bytes is None else ws_bytes, DEV)
    extra = [None if drop == i else x.data_ptr() for i, x in enumerate((same, other, held))]
    st = lib.taoamd_track_error_types_links(
        n_dt, n_gt, f.n_cells, len(iou), n_vid, K, n_rng, slot, tb,
        *[c.data_ptr() for c in cols], np.asarray(mg).reshape(rows, -1).shape[1],
        *[c.data_ptr() for c in gcols], *[c.data_ptr() for c in fr],
        *[c.data_ptr() for c in lists], dt_counts.data_ptr(), gt_counts.data_ptr(),
        dt_type.data_ptr(), dt_over.data_ptr(), *extra, ws.data_ptr(), ws.nbytes, _stream())
    if status:
        torch.cuda.synchronize()
        return st
    _lib.check(st, "taoamd_track_error_types_links")
    ws.check()
    return dict(dt_counts=dt_counts.cpu().numpy(), gt_counts=gt_counts.cpu().numpy(),
                dt_type=dt_type[:n_dt].cpu().numpy(),
                dt_over=dt_over[:n_dt].cpu().numpy().view(np.uint32),
                link_same=same[:n_dt].cpu().numpy(), link_other=other[:n_dt].cpu().numpy(),
                held=held[:, :n_gt].cpu().numpy())


def _same_pass(got, want):
    """links, held, types and counts (_same_links of the image level) and the masks"""
    _same_links(got, want)
    assert np.array_equal(got["dt_over"], want["types"]["dt_over"])


def _device_impact(n_cat, n_rng, dt_cat, score, dt_type, link_same, link_other, gt_cat, gt_rng,
                   held, status=False, ws_bytes=None):
    """taoamd_track_error_impact on bare tables, cat_off / order[] as the sort
    leaves them; the workspace is exactly the size reported, behind a guard band."""
    import torch
    lib = _lib.load()
    n_dt, n_gt = len(dt_cat), len(gt_cat)
    width = max(n_rng, 1)
    cat_off, srt = imp_ref.sweep_order(dt_cat, score, n_cat)
    cols = [_up(cat_off, np.int32), _up(srt, np.int32), _up(score, np.float64),
            _up(dt_cat, np.int32), _up(np.asarray(dt_type).reshape(n_dt, -1)
                                      if n_dt else np.zeros((0, width)), np.uint8),
            _up(np.asarray(link_same).reshape(n_dt, -1) if n_dt else np.zeros((0, width)),
                np.int32),
            _up(np.asarray(link_other).reshape(n_dt, -1) if n_dt else np.zeros((0, width)),
                np.int32),
            _up(gt_cat, np.int32), _up(gt_rng, np.uint32).view(torch.int32),
            _up(np.asarray(held).reshape(-1, n_gt) if n_gt else np.zeros((width, 0)), np.uint8)]
    P = torch.full((9, N_REC, n_cat, width), -7.0, dtype=torch.float64, device=DEV)
    NG = torch.full((9, n_cat, width), -7, dtype=torch.int32, device=DEV)
    need = lib.taoamd_track_error_impact_workspace(n_dt, n_gt, n_cat, min(width, 20))
    ws = wsguard.Guarded(need if ws_bytes is None else ws_bytes, DEV)
    st = lib.taoamd_track_error_impact(
        n_dt, n_gt, n_cat, n_rng, *[c.data_ptr() for c in cols], P.data_ptr(), NG.data_ptr(),
        ws.data_ptr(), ws.nbytes, _stream())
    if status:
        torch.cuda.synchronize()
        return st
    _lib.check(st, "taoamd_track_error_impact")
    ws.check()
    return dict(precision=P.cpu().numpy(), num_gt=NG.cpu().numpy().astype(np.int64))


def _impact_of(f, types, gt_rng, n_rng):
    return _device_impact(len(f.cat_ids), n_rng, f.dt_cat, f.dt_score, types["dt_type"],
                          types["link_same"], types["link_other"], f.gt_cat, gt_rng,
                          types["held"])


def _frozen(want):
    for v in list(want.values()) + list(want["types"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return want


def _tables_of(f, n_rng):
    gt_rng, dt_rng = orclib.ranges(f)
    with np.errstate(all="ignore"):
        iou, _ = orclib.track_iou(f)
    mg = _device_match(f, iou, gt_rng, dt_rng, n_rng)
    return iou, gt_rng, dt_rng, mg


# ---------------------------------------------------------------------------
# the links pass, then the sweep on its tables
# ---------------------------------------------------------------------------
def test_abi_on_the_hand_written_table():
    f, dt_at, gt_at = te.hand_flat()
    iou, gt_rng, dt_rng, mg = _tables_of(f, 20)
    thrs, rec = orclib.thresholds()
    want = ref.error_impact(f, iou, mg, gt_rng, dt_rng, thrs, 0, te.HAND_TB)
    got = _device_links(f, iou, mg, gt_rng, dt_rng, 20, 0, te.HAND_TB)
    # the literals of the host test, from the device
    assert got["dt_type"][dt_at, 0].tolist() == te.HAND_TYPES_RNG0
    assert got["link_same"][dt_at[[3, 9, 13, 15]], 0].tolist() == gt_at[[2, 5, 6, 8]].tolist()
    assert got["link_other"][dt_at[[4, 10, 5, 11, 12]], 0].tolist() == \
        gt_at[[3, 4, 3, 5, 4]].tolist()
    assert got["link_same"][dt_at[15], [0, 1, 3]].tolist() == [gt_at[8], -1, gt_at[8]]
    assert (got["link_other"][dt_at[16]] == -1).all()
    assert got["held"][0, gt_at].tolist() == [1, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    _same_pass(got, want)
    imp = _impact_of(f, got, gt_rng, 20)
    P = imp["precision"][..., 0]
    assert np.array_equal(P[ref.F_LOC, :, 0], img.hand.expected(
        7, {**{c: (5, 5) for c in range(6)}, 6: (7, 10), 7: (7, 10)}, rec))
    assert np.array_equal(P[ref.F_CLS, :, 1], img.hand.expected(1, {0: (1, 2), 1: (1, 2)}, rec))
    assert imp["num_gt"][ref.F_FN, :, 0].tolist() == [3, 0, 0]
    _same(imp, want)


@pytest.fixture(scope="module")
def seeded_tables():
    """{n_rng: (flat, iou, gt_rng, dt_rng, match_gt of taoamd_match, {(slot, tb):
    restatement})} on the tables of the breakdown's own test."""
    out = {}
    thrs, _ = orclib.thresholds()
    for n_rng in (1, 20):
        f = _seeded_table(50 + n_rng)
        iou, gt_rng, dt_rng, mg = _tables_of(f, n_rng)
        want = {(t, tb): _frozen(ref.error_impact(f, iou, mg, gt_rng, dt_rng, thrs, t, tb, n_rng))
                for t, tb in SETTINGS}
        out[n_rng] = (f, iou, gt_rng, dt_rng, mg, want)
    return out


@pytest.mark.parametrize("slot,tb", SETTINGS)
@pytest.mark.parametrize("n_rng", [1, 20])
def test_links_and_sweep_on_seeded_tables(seeded_tables, n_rng, slot, tb):
    f, iou, gt_rng, dt_rng, mg, want = seeded_tables[n_rng]
    w = want[slot, tb]
    # the cases are there.  (tb = 0: an unmatched row is DUP or LOC: no CLS row,
    # none adopted)
    assert w["events"]["winner"] > 0 and w["events"]["lost_to_held"] > 0
    assert (w["events"]["adopted"] > 0) == (tb > 0)
    assert (w["link_same"] == -1).any() and (w["link_same"] >= 0).any()
    assert (w["link_other"] == -1).any() and (w["link_other"] >= 0).any()
    # links of another category, whatever the row's type
    linked = w["link_other"][:, 0] >= 0
    assert (np.asarray(f.gt_cat)[w["link_other"][linked, 0]] != np.asarray(f.dt_cat)[linked]).all()
    assert set(np.unique(w["types"]["dt_type"][linked])) >= {te.TP, te.DUP, te.LOC}
    got = _device_links(f, iou, mg, gt_rng, dt_rng, n_rng, slot, tb)
    _same_pass(got, w)
    _same(_impact_of(f, got, gt_rng, n_rng), w)


# (ground-truth tracks, detection tracks) per video: around the tile of
# ground-truth tracks (TE_G) x around a round of lanes (TE_LANES); a video without
# ground truth; a video whose ground truths all share the detections' category
EDGE_VIDEOS = [(g, d) for g in (1, TILE, TILE + 1, 2 * TILE + 1) for d in (1, LANES, LANES + 1)] \
    + [(0, 5), (TILE, 64)]
NO_GT_VIDEO, ONE_CAT_VIDEO = len(EDGE_VIDEOS) - 2, len(EDGE_VIDEOS) - 1


def _edge_table(seed, boxes=None):
    """_seeded_table of the breakdown's test on EDGE_VIDEOS."""
    keep = trk.VIDEOS, trk.ONE_CAT_VIDEO
    trk.VIDEOS, trk.ONE_CAT_VIDEO = EDGE_VIDEOS, ONE_CAT_VIDEO
    try:
        return _seeded_table(seed, boxes)
    finally:
        trk.VIDEOS, trk.ONE_CAT_VIDEO = keep


def test_links_at_every_edge_of_the_pair_kernel():
    f = _edge_table(7)
    n_dt = int(f.cell_dt_off[-1])
    assert n_dt == sum(d for _, d in EDGE_VIDEOS) < 3000
    d_vid, g_vid = te.units(f)
    assert np.bincount(g_vid, minlength=len(EDGE_VIDEOS)).tolist() == [g for g, _ in EDGE_VIDEOS]
    # a detection track that starts mid-chunk and spans three or more chunks of 8
    off, pos = np.asarray(f.dt_frame_off), np.asarray(f.dt_frame_pos)
    first, last = pos[off[:-1]], pos[off[1:] - 1]
    assert ((first % CHUNK_POS != 0) & ((last // CHUNK_POS) - (first // CHUNK_POS) >= 2)).any()
    iou, gt_rng, dt_rng, mg = _tables_of(f, 20)
    thrs, _ = orclib.thresholds()
    want = ref.error_impact(f, iou, mg, gt_rng, dt_rng, thrs, 0, 0.1)
    lo = want["link_other"]
    # nothing to link without ground truth, nor where it is all of the row's category
    assert (lo[d_vid == NO_GT_VIDEO] == -1).all()
    one = (d_vid == ONE_CAT_VIDEO) & (np.asarray(f.dt_cat) == 0)
    assert one.any() and (lo[one] == -1).all()
    # every video with a tile of ground truth or more links some row; where it
    # has 257 detection tracks, the one of the second round of lanes is linked too
    for v, (g, d) in enumerate(EDGE_VIDEOS):
        if g >= TILE and v != ONE_CAT_VIDEO:
            assert (lo[d_vid == v] >= 0).any(), v
    last = np.array([np.flatnonzero(d_vid == v)[-1] for v, (g, d) in enumerate(EDGE_VIDEOS)
                     if d == LANES + 1])
    assert (lo[last] >= 0).any()
    got = _device_links(f, iou, mg, gt_rng, dt_rng, 20, 0, 0.1)
    _same_pass(got, want)
    _same(_impact_of(f, got, gt_rng, 20), want)


def _still(box, positions=(0, 1, 2)):
    return {p: list(box) for p in positions}


def _special_table():
    """Video 0: 24 ground-truth tracks of category 1 (their table rows ascend in
    the order given, which is the video's list), those at list positions 3 and 19
    with identical frames (tiles 0 and 1), those at 5 and 7 too (one tile).
    Video 1: one ground-truth track of category 1 whose boxes are disjoint from
    the detection's: IoU exactly 0.  Video 2: one whose sums of i and of u both
    overflow (1e308 a frame, three frames): IoU inf / inf, a NaN.  Video 3:
    a long one (12 frames: evaluated in slots 0 and 3, ignored in 1 and 2)."""
    gts = []
    for i in range(24):
        box = [40 * i, 0, 10, 4 + i % 3]
        if i in (3, 19):
            box = [1000, 0, 10, 10]
        if i in (5, 7):
            box = [2000, 0, 10, 10]
        gts.append((0, 1, _still(box), 0))
    gts += [(1, 1, _still([100, 0, 10, 10]), 0),
            (2, 1, _still([0, 0, 1e154, 1e154]), 0),
            (3, 1, _still([0, 0, 10, 10], range(12)), 0)]
    dets = [(0, 0, _still([1000, 0, 10, 10]), 0.9, 0),      # 0  IoU 1 with gt 3 and gt 19
            (0, 0, _still([2000, 0, 10, 8]), 0.8, 0),       # 1  IoU 0.8 with gt 5 and gt 7
            (0, 2, _still([5000, 0, 10, 10]), 0.7, 0),      # 2  IoU 0 with all 24: the first
            (1, 0, _still([0, 0, 10, 10]), 0.9, 0),         # 3  IoU 0, the only candidate
            (2, 0, _still([0, 0, 1e154, 1e154]), 0.9, 0),   # 4  IoU NaN alone
            (3, 0, _still([0, 0, 10, 10]), 0.9, 0)]         # 5  IoU 3 / 12
    return te.make_track_flat(4, 3, dets, gts)


@pytest.mark.parametrize("reverse", [False, True])
def test_links_ties_zero_nan_and_ignored_ranges(reverse):
    f, dt_at, gt_at = _special_table()
    assert gt_at[:24].tolist() == list(range(24))          # list position = table row
    iou, gt_rng, dt_rng, mg = _tables_of(f, 20)
    with np.errstate(all="ignore"):
        blocks = {int(D[0]): m for D, _, m in te.cross_blocks(f)}
    m0 = blocks[int(min(dt_at[:3]))]
    assert m0.shape == (3, 24)
    # bit-equal IoUs of the tied pairs
    assert (m0[:, 3] == m0[:, 19]).all() and (m0[:, 5] == m0[:, 7]).all()
    assert m0[:, 3].max() == 1.0 and m0[:, 5].max() == 0.8 and (m0.min(1) == 0).all()
    d_vid, g_vid = te.units(f)
    g_off, g_rows = _csr(g_vid, 4)
    d_off, d_rows = _csr(d_vid, 4)
    assert g_rows[:24].tolist() == list(range(24))
    if reverse:
        g_rows = g_rows.copy()
        g_rows[:24] = g_rows[:24][::-1]                    # row 19 comes at position 4, row 3 at 20
    thrs, _ = orclib.thresholds()
    with np.errstate(all="ignore"):
        want = ref.error_impact(f, iou, mg, gt_rng, dt_rng, thrs, 0, 0.1)
    got = _device_links(f, iou, mg, gt_rng, dt_rng, 20, 0, 0.1,
                        lists=(g_off, g_rows, d_off, d_rows))
    lo = got["link_other"]
    # the lower table row wins, in two tiles and in one, whatever the list's order
    assert lo[dt_at[0], 0] == gt_at[3] and lo[dt_at[1], 0] == gt_at[5]
    assert lo[dt_at[2], 0] == gt_at[0]
    # an IoU of exactly 0 that is the only candidate is the link
    assert lo[dt_at[3], 0] == gt_at[24]
    # overlaps that are NaN alone link nothing
    assert np.isnan(blocks[int(dt_at[4])]).all() and (lo[dt_at[4]] == -1).all()
    # ignored in slots 1 and 2 (a long track), evaluated in 0 and 3
    assert lo[dt_at[5], :4].tolist() == [gt_at[26], -1, -1, gt_at[26]]
    _same_pass(got, want)
    _same(_impact_of(f, got, gt_rng, 20), want)


def test_links_on_boxes_that_are_any_double():
    """Coordinates from every population of tests/boxpop.py: a NaN IoU is no
    overlap, a row whose only overlaps are NaN links nothing."""
    prng = np.random.default_rng(77)
    turn = [0]

    def boxes(n):
        kind = boxpop.KINDS[turn[0] % len(boxpop.KINDS)]
        turn[0] += 1
        return boxpop.box_population(kind, 2 * n, prng)
    # (seed 97: five rows of the table have candidates in range 0 that are all NaN)
    f = _edge_table(97, boxes)
    iou, gt_rng, dt_rng, mg = _tables_of(f, 20)
    thrs, _ = orclib.thresholds()
    dt_cat, gt_cat = np.asarray(f.dt_cat), np.asarray(f.gt_cat)
    with np.errstate(all="ignore"):
        want = ref.error_impact(f, iou, mg, gt_rng, dt_rng, thrs, 0, 0.1)
        # rows with candidates in range 0, every one of them a NaN
        lone = []
        for D, G, m in te.cross_blocks(f):
            cand = (dt_cat[D][:, None] != gt_cat[G][None, :]) & ((gt_rng[G] & 1) == 0)[None, :]
            lone += D[cand.any(1) & (np.isnan(m) | ~cand).all(1)].tolist()
    assert lone and (want["link_other"][lone, 0] == -1).all()
    assert np.isnan(iou).any() and (want["link_other"] >= 0).any()
    got = _device_links(f, iou, mg, gt_rng, dt_rng, 20, 0, 0.1)
    _same_pass(got, want)
    assert (got["link_other"][lone, 0] == -1).all()


def test_links_skip_rows_outside_the_tables(seeded_tables):
    """A vid_dt entry >= n_dt or a vid_gt entry < 0 (and their like): such a
    detection row is listed nowhere and links nothing of another category, such
    a ground truth is in no video's set.  Nothing is dereferenced."""
    f, iou, gt_rng, dt_rng, mg, _ = seeded_tables[20]
    n_dt, n_gt, n_vid = int(f.cell_dt_off[-1]), int(f.cell_gt_off[-1]), len(f.vid_ids)
    thrs, _ = orclib.thresholds()
    rng = np.random.default_rng(5)
    d_vid, g_vid = te.units(f)
    g_off, g_rows = _csr(g_vid, n_vid)
    d_off, d_rows = _csr(d_vid, n_vid)
    g_bad = rng.choice(n_gt, 25, replace=False)
    d_bad = rng.choice(n_dt, 60, replace=False)
    g_junk = np.array([n_gt, n_gt + 7, 2 ** 31 - 1, -1, -2 ** 31])
    # (every entry outside [0, n_dt): a row two videos list would be written by both)
    d_junk = np.array([n_dt, n_dt + 7, 2 ** 31 - 1, -1, -2 ** 31])
    g_rows, d_rows = g_rows.copy(), d_rows.copy()
    g_rows[np.isin(g_rows, g_bad)] = g_junk[np.arange(25) % 5]
    d_rows[np.isin(d_rows, d_bad)] = d_junk[np.arange(60) % 5]
    mg2 = mg.copy()
    m_bad = rng.random(mg.shape) < 0.02
    mg2[m_bad] = rng.choice([10 ** 6, 2 ** 31 - 1, -5, -2 ** 31], int(m_bad.sum()))
    gl, dl = np.ones(n_gt, bool), np.ones(n_dt, bool)
    gl[g_bad], dl[d_bad] = False, False
    want = ref.error_impact(f, iou, mg2, gt_rng, dt_rng, thrs, 0, 0.1, dt_listed=dl, gt_listed=gl)
    got = _device_links(f, iou, mg2, gt_rng, dt_rng, 20, 0, 0.1,
                        lists=(g_off, g_rows, d_off, d_rows))
    _same_pass(got, want)
    assert (got["link_other"][d_bad] == -1).all() and (got["link_same"][d_bad] >= 0).any()
    assert not np.isin(got["link_other"], g_bad).any()


def test_error_types_outputs_unchanged_after_a_links_call(seeded_tables):
    f, iou, gt_rng, dt_rng, mg, want = seeded_tables[20]
    plain = lambda: trk._device_error_types(f, iou, mg, gt_rng, dt_rng, 20, 0, 0.1)  # noqa: E731
    before = plain()
    _device_links(f, iou, mg, gt_rng, dt_rng, 20, 5, 0.25)
    after = plain()
    for k in ("dt_counts", "gt_counts", "dt_type", "dt_over"):
        assert np.array_equal(before[k], after[k])
        assert np.array_equal(before[k], want[0, 0.1]["types"][k])


def test_links_with_the_workspace_base_moved_by_8_bytes(seeded_tables, monkeypatch):
    monkeypatch.setattr(wsguard, "SHIFT", 8)
    f, iou, gt_rng, dt_rng, mg, want = seeded_tables[20]
    _same_pass(_device_links(f, iou, mg, gt_rng, dt_rng, 20, 5, 0.25), want[5, 0.25])


def test_links_error_paths(seeded_tables):
    f, iou, gt_rng, dt_rng, mg, _ = seeded_tables[1]
    lib = _lib.load()
    call = lambda **kw: _device_links(                                      # noqa: E731
        f, iou, mg, gt_rng, dt_rng, kw.pop("n_rng", 1), kw.pop("slot", 0), kw.pop("tb", 0.1),
        status=True, **kw)
    assert call(drop=0) == 2 and call(drop=1) == 2 and call(drop=2) == 2
    assert call(slot=10) == 2 and call(tb=0.5) == 2 and call(tb=0.9) == 2
    assert call(n_rng=21) == 2
    need = lib.taoamd_track_error_types_workspace(int(f.cell_dt_off[-1]),
                                                  int(f.cell_gt_off[-1]), 1)
    assert call(ws_bytes=need - 1) == 4
    assert call() == 0


# ---------------------------------------------------------------------------
# the sweep on bare tables: up to 20 ranges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_rng", [9, 20])
def test_sweep_on_seeded_bare_tables(n_rng):
    t = bare_tables(n_rng)
    want = imp_ref.impact_tables(rec_thrs=orclib.thresholds()[1], **t)
    for name in img.EVENTS:
        assert want["events"][name] > 0, name
    # a category of 513 rows: two carries across steps of 256 rows
    assert np.bincount(t["dt_cat"], minlength=t["n_cat"]).max() == 2 * img.CHUNK + 1
    for v in range(1, 9):
        assert (want["precision"][v] != want["precision"][0]).any(), imp_ref.FIXES[v]
    # the ranges past the image level's eight are swept like the others
    assert (want["precision"][..., 8:] > 0).any() and (want["num_gt"][..., n_rng - 1] > 0).any()
    _same(_device_impact(**t), want)


def test_sweep_without_rows_or_ground_truths():
    rec = orclib.thresholds()[1]
    n_rng = 20
    none = np.zeros((0, n_rng), np.int64)
    t = dict(n_cat=3, n_rng=n_rng, dt_cat=np.zeros(0, np.int64), score=np.zeros(0),
             dt_type=np.zeros((0, n_rng), np.uint8), link_same=none, link_other=none,
             gt_cat=np.array([0, 0, 2]), gt_rng=np.array([0, 1 | 1 << 19, 0], np.uint32),
             held=np.zeros((n_rng, 3), bool))
    got = _device_impact(**t)
    _same(got, imp_ref.impact_tables(rec_thrs=rec, **t))
    assert got["num_gt"][0, :, 0].tolist() == [1, 0, 1] and got["num_gt"][0, :, 1].tolist() == \
        [2, 0, 1] and got["num_gt"][0, :, 19].tolist() == [1, 0, 1]
    assert (got["precision"][0, :, 0] == 0).all() and (got["precision"][0, :, 1] == -1).all()
    t.update(gt_cat=np.zeros(0, np.int64), gt_rng=np.zeros(0, np.uint32),
             held=np.zeros((n_rng, 0), bool), dt_cat=np.array([1, 1]), score=np.array([0.5, 0.25]),
             dt_type=np.repeat(np.array([[0], [6]], np.uint8), n_rng, 1),
             link_same=-np.ones((2, n_rng), np.int64), link_other=-np.ones((2, n_rng), np.int64))
    got = _device_impact(**t)
    _same(got, imp_ref.impact_tables(rec_thrs=rec, **t))
    assert (got["precision"] == -1).all()


def test_sweep_error_paths_and_the_image_levels_limit():
    t = bare_tables(1)
    lib = _lib.load()
    assert _device_impact(status=True, **t) == 0
    assert _device_impact(status=True, ws_bytes=lib.taoamd_track_error_impact_workspace(
        len(t["dt_cat"]), len(t["gt_cat"]), t["n_cat"], 1) - 1, **t) == 4
    assert _device_impact(status=True, **{**t, "n_rng": 0}) == 2
    assert _device_impact(status=True, **{**t, "n_rng": 21}) == 2
    # the image level's entry keeps its eight ranges
    assert img._device_impact(status=True, **bare_tables(9)) == 2


def test_sweep_at_six_ranges_is_the_image_levels_bit_for_bit():
    t = bare_tables(6)
    ours, theirs = _device_impact(**t), img._device_impact(**t)
    assert np.array_equal(ours["precision"].view(np.uint64), theirs["precision"].view(np.uint64))
    assert np.array_equal(ours["num_gt"], theirs["num_gt"])
    assert (ours["precision"] > 0).any()


# ---------------------------------------------------------------------------
# the class API
# ---------------------------------------------------------------------------
FIXTURES = ["f1", "f2", "f3", "f4", "f5", "f7", "f9", "f10", "f11"]
HIDDEN_IDS = ("f2", "f9")       # the fixtures with a ground-truth track whose id is hidden
GT_ID_HIDDEN = 4


def _restated(ev, iou_thr, bg_thr):
    """The restatement on the evaluator's own tables (as _restated of the
    breakdown's test): IoU matrix, match indices and range masks of a
    detail-mode pass under the evaluator's constants, the kernels' range slots
    put in the caller's order, the recall thresholds the caller's."""
    import torch
    from tao_amodal_amd import engine
    from tao_amodal_amd.evaluation._core import applied
    run = ev._run
    c = run.constants
    ws = engine.Workspace(run.dp, detail=True)
    with applied(c):
        engine.run_guarded(run.dp, ws, run.flat, upto="match")
        torch.cuda.synchronize()
    n_dt, n_gt = run.dp.n_dt, run.dp.n_gt
    mg = ws.match_gt[:n_dt].cpu().numpy()
    gt_rng = ws.gt_rng[:n_gt].cpu().numpy().view(np.uint32)
    dt_rng = ws.dt_rng[:n_dt].cpu().numpy().view(np.uint32)
    iou = ws.iou[:run.dp.n_iou].cpu().numpy()
    thrs = orclib.thresholds()[0] if c is None else c.thr_blocks[0][1]
    i = int(np.where(iou_thr == np.asarray(ev.params.iou_thrs))[0][0])
    slot = i if c is None else int(np.where(c.thr_blocks[0][0] == i)[0][0])
    assert thrs[slot] == iou_thr
    want = ref.error_impact(run.flat, iou, mg, gt_rng, dt_rng, thrs, slot, bg_thr,
                            rec_thrs=np.asarray(ev.params.rec_thrs, dtype=np.float64))
    P = want["precision"]
    A, T = len(ev.params.area_rng), len(ev.params.time_rng)
    if (A, T) != (5, 4):
        ks = [(a if a < A - 1 else 4) * 4 + t for a in range(A) for t in range(T)]
        P = P[..., ks]
    cats = np.asarray(run.flat.cat_ids).tolist()
    pos = [cats.index(int(c)) for c in ev.params.cat_ids]
    hidden = np.zeros(len(cats), bool)
    hidden[np.asarray(run.flat.gt_cat)[(np.asarray(run.flat.gt_flags) & GT_ID_HIDDEN) != 0]] = True
    return np.ascontiguousarray(P[:, :, pos]), want["events"], hidden[pos]


def _check_class_api(ev, iou_thr, bg_thr, monkeypatch):
    from tao_amodal_amd.evaluation._core import masked_mean
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.error_impact(iou_thr, bg_thr)
    ev.evaluate()
    want, events, hidden = _restated(ev, iou_thr, bg_thr)
    calls = []
    table = ev._run.impact_table
    monkeypatch.setattr(ev._run, "impact_table", lambda *a: calls.append(a) or table(*a))
    got = ev.error_impact(iou_thr, bg_thr)
    P = ev.params
    A, T = len(P.area_rng), len(P.time_rng)
    n_rng, K, R = A * T, len(P.cat_ids), len(P.rec_thrs)
    assert got["fixes"] == list(ref.FIXES)
    assert got["rng_lbl"] == ev.error_types(iou_thr, bg_thr)["rng_lbl"]
    assert len(got["rng_lbl"]) == n_rng and got["rng_lbl"][0] == ("all", "all")
    assert got["precision"].shape == (9, R, K, n_rng) and got["precision"].dtype == np.float64
    assert np.array_equal(got["precision"], want)
    assert got["ap"].shape == (9, n_rng) and got["dap"].shape == (8, n_rng)
    for v in range(9):
        for a in range(n_rng):
            assert got["ap"][v, a] == masked_mean(want[v, :, :, a])
    assert np.array_equal(got["dap"], got["ap"][1:] - got["ap"][0])
    # a second call: the cache, equal arrays and no kernel launched
    again = ev.error_impact(iou_thr, bg_thr)
    assert len(calls) == 1 and again["precision"] is got["precision"]
    assert np.array_equal(again["ap"], got["ap"]) and np.array_equal(again["dap"], got["dap"])
    # BASE is accumulate()'s table at the threshold, hidden-id categories set aside
    ev.accumulate()
    t = int(np.where(iou_thr == np.asarray(P.iou_thrs))[0][0])
    base = got["precision"][0].reshape(R, K, A, T)
    assert np.array_equal(base[:, ~hidden], ev.eval["precision"][t][:, ~hidden])
    lines = ev.impact_lines(iou_thr, bg_thr)
    assert len(lines) == 2 + n_rng and all(isinstance(x, str) for x in lines)
    assert lines[1].split() == ["AP"] + ["d" + x for x in ref.FIXES[1:]]
    assert lines[2].split()[0] == "all/all"
    assert lines[2].split()[-9:] == ["%.4f" % v for v in
                                     np.concatenate([got["ap"][:1, 0], got["dap"][:, 0]])]
    assert len(calls) == 1
    return got, events, hidden


@pytest.mark.parametrize("name", FIXTURES)
def test_class_api_on_the_fixtures(name, tmp_path, monkeypatch):
    ev = trk._tao(name, tmp_path)
    got, _, hidden = _check_class_api(ev, 0.5, 0.1, monkeypatch)
    # the cap on what is set aside: nothing, but on the two fixtures with hidden ids
    assert hidden.any() == (name in HIDDEN_IDS)
    if not hidden.any():
        # its mean is the AP summarize() reports at the threshold
        assert got["ap"][0, 0] == ev._summarize("ap", 0.5, "all", "all")


def test_class_api_at_another_threshold(monkeypatch):
    ev = trk._tao("f1")
    got, events, _ = _check_class_api(ev, 0.75, 0.3, monkeypatch)
    assert ev.params.iou_thrs[5] == 0.75 and events["winner"] > 0


@pytest.mark.parametrize("case,iou_thr", [("few", 0.75), ("few", 0.3), ("ranges3", 0.5)])
def test_class_api_under_edited_constants_of_one_block(case, iou_thr, monkeypatch):
    """Thresholds in the caller's unsorted order and 11 recall thresholds; 3 area
    ranges x 2 durations (kernel slots 0, 1 and the occlusion one; 0 and 1)."""
    ev = trk._tao("f1")
    edit(ev.params, cases()[case], "tao")
    got, _, _ = _check_class_api(ev, iou_thr, 0.1, monkeypatch)
    assert got["precision"].shape[3] == len(ev.params.area_rng) * len(ev.params.time_rng)
    assert got["precision"].shape[1] == len(ev.params.rec_thrs)


def test_class_api_on_a_params_subset(monkeypatch):
    ev = trk._tao("f1")
    ev.params.vid_ids = ev.params.vid_ids[::2]
    ev.params.cat_ids = [ev.params.cat_ids[i] for i in (4, 0, 2)]
    got, _, _ = _check_class_api(ev, 0.5, 0.1, monkeypatch)
    assert got["precision"].shape[2] == 3 and (got["precision"] > 0).any()


def test_class_api_refusals():
    from goldenio import path
    ev = trk._tao("f1")
    ev.evaluate()
    with pytest.raises(ValueError, match="not one of params.iou_thrs"):
        ev.error_impact(0.55000001)
    for bad in (0.5, 0.7, -0.1):
        with pytest.raises(ValueError, match="bg_thr"):
            ev.error_impact(0.5, bad)
    from tao_amodal_amd import engine
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_track_error_impact(ev._run.dp, ev._run.ws, 10, 0.1)
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_track_error_impact(ev._run.dp, ev._run.ws, 0, 0.5)
    with pytest.raises(_lib.TaoAmdError, match="track level's"):
        engine.stage_track_error_impact(trk._lvis_run().dp, trk._lvis_run().ws, 0, 0.1)
    many = trk._tao("f1")
    edit(many.params, cases()["many"], "tao")
    many.evaluate()
    with pytest.raises(NotImplementedError, match=r"error_types\(\) is kept for up to 10 IoU"):
        many.error_impact(many.params.iou_thrs[9])
    wide = trk._tao("f1")
    edit(wide.params, cases()["ranges8"], "tao")
    wide.evaluate()
    with pytest.raises(NotImplementedError, match="one block of ranges"):
        wide.error_impact(0.5)
    fine = trk._tao("f1")
    fine.params.rec_thrs = np.linspace(0.0, 1.0, 201)
    fine.evaluate()
    with pytest.raises(NotImplementedError, match=r"error_impact\(\) is kept for up to 101 recall"):
        fine.error_impact(0.5)
    pooled = trk._tao("f1")
    pooled.params.use_cats = 0
    pooled.evaluate()
    with pytest.raises(NotImplementedError, match="use_cats = 0"):
        pooled.error_impact(0.5)
    avg = trk._tao("f1", iou_3d_type="avg_iou")
    avg.evaluate()
    with pytest.raises(NotImplementedError, match="iou_3d_type='avg_iou'"):
        avg.error_impact(0.5)
    with pytest.raises(_lib.TaoAmdError, match="3d_iou"):
        engine.stage_track_error_impact(avg._run.dp, avg._run.ws, 0, 0.1)
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval
    segm = TaoEval(Tao(path("f6", "gt.json")), path("f6", "pred_rle.json"), iou_type="segm")
    segm.evaluate()
    with pytest.raises(NotImplementedError, match="iou_type='segm'"):
        segm.error_impact(0.5)
    from tao_amodal_amd.evaluation._dist import DistRun
    with pytest.raises(NotImplementedError, match=r"error_types\(\) in a multi-GPU run"):
        DistRun.__new__(DistRun).impact_table(0, 0.1)


def test_image_level_error_impact_is_unchanged():
    """LVISEval.error_impact() on f1 against the image level's restatement, by
    the image level's own check."""
    got, events = img._check_class_api(img._lvis("f1", None, pred="pred.json"), 0.5, 0.1)
    assert got["precision"].shape[3] == 6 and events["winner"] > 0
