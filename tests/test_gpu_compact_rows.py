"""The image level's 4-byte match rows (taoamd_match_compact, taoamd_expand_rows,
taoamd_accumulate_by_order_compact; engine.Workspace's lazily expanding views).

Where no detection of a cell overlaps two ground truths by the lowest threshold
a row of the gathered chain is a function of 18 bits: the ten threshold bits
m10, the candidate's 6-bit range mask g, "ignored when unmatched" u and "the
candidate is hidden" h, with
    matched = h ? 0 : m10 * S(all),   ignored = m10 * S(g) | X * (u ? S(all) : 0),
    X = h ? 0x3ff : ~m10 & 0x3ff,     S(g) = sum of 2^(10 q) over the bits q of g
(csrc/iou_match.hip).  The match stores that word, the sweep expands it with
shifts and a table of masks, and a row the sequential greedy produced is
escaped (bit 31) to the 16-byte row table.  Checked here: the table form
against the products over all 2^18 words (host, numpy); the expand kernel over
the same words; compact match rows against the non-compact instance and the C
oracle on the long-category problem, on cells whose detections overlap two
ground truths and on a hand-built set of runs that mix both paths; the compact
sweep on every boundary of its blocking with escaped rows mixed in, under the
look-back and behind a counting pass; a look-back that gives up; and compact
and scatter passes alternating on one workspace.
Reference: lvis_amodal/eval.py:225-337 (match), 339-426 (accumulate)."""
import ctypes as C
import functools

import numpy as np
import pytest

import orclib
import wsguard
from tao_amodal_amd import _lib
from tao_amodal_amd import flatten as fl
from tao_amodal_amd.columns import DTColumns, GTColumns
from tao_amodal_amd.synth import synth

gpu = pytest.mark.gpu

N_THR, N_REC = _lib.N_THR, _lib.N_REC
ESCAPE = np.uint32(0x80000000)
SC = 2048                       # rows of a super-chunk (4 wavefronts x 512)
CHUNK = 512                     # rows of a wavefront's chunk
U64 = np.uint64


# ---------------------------------------------------------------------------
# the word and its two expansions, in numpy
# ---------------------------------------------------------------------------
def _S(g):
    """S(g): bit 10 q for every set bit q of the 6-bit mask g."""
    g = np.asarray(g, U64)
    out = np.zeros(g.shape, U64)
    for q in range(6):
        out |= ((g >> U64(q)) & U64(1)) << U64(10 * q)
    return out


def _fields(w, n_rng):
    w = np.asarray(w, np.uint32)
    rmask = np.uint32((1 << n_rng) - 1)
    return ((w & np.uint32(0x3ff)).astype(U64), (w >> np.uint32(10)) & rmask,
            ((w >> np.uint32(16)) & np.uint32(1)).astype(bool),
            ((w >> np.uint32(17)) & np.uint32(1)).astype(bool), U64(int(rmask)))


def expand_products(w, n_rng=6):
    """(matched, ignored) of the words w by the match kernel's products."""
    m10, g, u, h, rmask = _fields(w, n_rng)
    sall = _S(rmask)
    X = np.where(h, U64(0x3ff), ~m10 & U64(0x3ff))
    matched = np.where(h, U64(0), m10 * sall)
    ignored = m10 * _S(g) | np.where(u, X * sall, U64(0))
    return matched, ignored


def expand_tables(w, n_rng=6):
    """(TP, valid) of the words w as the sweep works them out: the threshold
    bits repeated six times by shift-or, the pair (T, ~A) from a 256-entry table
    keyed by bits 10-17, ~B from bit 16 (csrc/accumulate.hip, crow_expand)."""
    w = np.asarray(w, np.uint32)
    rmask = (1 << n_rng) - 1
    all_ = int(_S(U64(rmask))) * 0x3ff
    T, nA = np.zeros(256, U64), np.zeros(256, U64)
    full = (1 << 64) - 1
    for key in range(256):
        g, u, h = key & 63 & rmask, (key >> 6) & 1, (key >> 7) & 1
        A = all_ if (h and u) else int(_S(U64(g))) * 0x3ff
        T[key] = (0 if h else all_) & ~A & full
        nA[key] = ~A & full
    m10 = w & np.uint32(0x3ff)
    lo = m10 | m10 << np.uint32(10)
    lo = lo | lo << np.uint32(20)                                  # (wraps at 32 bits)
    hi = m10 >> np.uint32(2) | m10 << np.uint32(8) | m10 << np.uint32(18)
    R = hi.astype(U64) << U64(32) | lo.astype(U64)
    key = (w >> np.uint32(10)) & np.uint32(255)
    nu = np.where((w >> np.uint32(16)) & np.uint32(1), U64(0), U64(full))
    nB = nu | U64(~all_ & full)
    return R & T[key], (R & nA[key]) | (~R & nB)


def test_the_table_form_equals_the_products_over_all_words():
    """Pack / expand identity over all 2^18 words, one to six ranges: TP =
    matched & ~ignored and valid = ~ignored of the products, bit for bit, and
    the fields read back from a packed word."""
    w = np.arange(1 << 18, dtype=np.uint32)
    for n_rng in range(1, 7):
        m, i = expand_products(w, n_rng)
        tp, valid = expand_tables(w, n_rng)
        assert np.array_equal(tp, m & ~i), n_rng
        assert np.array_equal(valid, ~i), n_rng
    m10, g, u, h, _ = _fields(w, 6)
    packed = (m10 | g.astype(U64) << U64(10) | u.astype(U64) << U64(16) |
              h.astype(U64) << U64(17)).astype(np.uint32)
    assert np.array_equal(packed, w)
    # the products against the loop over the ranges they replace
    rng = np.random.default_rng(1)
    for wk in rng.choice(w, 400, replace=False).tolist():
        m10k, gk, uk, hk = wk & 0x3ff, (wk >> 10) & 63, (wk >> 16) & 1, (wk >> 17) & 1
        mm = ii = 0
        for q in range(6):
            mm |= (0 if hk else m10k) << (10 * q)
            ib = (m10k if (gk >> q) & 1 else 0) | \
                ((0x3ff if hk else ~m10k & 0x3ff) if uk else 0)
            ii |= ib << (10 * q)
        assert (int(m[wk]), int(i[wk])) == (mm, ii), wk


# ---------------------------------------------------------------------------
# the expand kernel
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_rng", [6, 3, 1])
def test_expand_kernel_over_all_words(n_rng):
    """taoamd_expand_rows on every word, each once plain and once escaped: a
    plain word's row is the products', an escaped word's row is left alone."""
    import torch
    lib = _lib.load()
    w = np.arange(1 << 18, dtype=np.uint32)
    words = np.concatenate([w, w | ESCAPE])
    n = len(words)
    d_w = torch.from_numpy(words.view(np.int32)).to("cuda:0")
    rows = torch.full((n, 1, 2), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda:0")
    _lib.check(lib.taoamd_expand_rows(n, n_rng, d_w.data_ptr(), rows.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream),
               "taoamd_expand_rows")
    got = rows.cpu().numpy().view(U64).reshape(n, 2)
    m, i = expand_products(w, n_rng)
    assert np.array_equal(got[:len(w), 0], m) and np.array_equal(got[:len(w), 1], i)
    assert (got[len(w):] == U64(0x5a5a5a5a5a5a5a5a)).all()


# ---------------------------------------------------------------------------
# the match
# ---------------------------------------------------------------------------
@pytest.fixture
def gathering(monkeypatch):
    """The image level's production chain on a small problem: the sample sort
    and the one-pass sweep forced, so that a workspace gathers (and stores
    compact rows)."""
    from tao_amodal_amd import engine
    monkeypatch.setattr(engine, "_SORT_FORCE", "sampled")
    _lib.sweep_mode("lookback")
    yield engine
    _lib.sweep_mode("auto", spin_limit=0)


def _match_both_ways(engine, f, gt_rng=None):
    """Rows of the compact pass (expanded) and of the non-compact instance for
    the same cell tables, the compact words, and the oracle's rows."""
    import torch
    dp = engine.DeviceProblem(f, "cuda:0")
    assert engine.gathers_rows(dp)
    out = []
    for compact in (True, False):
        ws = engine.Workspace(dp)
        assert ws.gather and ws.compact_buf is not None
        ws.gather = compact
        ws.rows.fill_(-1)
        engine.stage_ranges(dp, ws)
        if gt_rng is not None:
            ws.gt_rng[:dp.n_gt] = torch.from_numpy(gt_rng.view(np.int32)).to("cuda:0")
        engine.stage_match(dp, ws, scatter=False)
        assert ws.cell_order and ws.rows_pending == compact
        n = dp.n_dt
        words = ws.compact_buf[:n].cpu().numpy().view(np.uint32) if compact else None
        if compact:
            # escaped rows are in the table before any expansion, the others untouched
            raw = ws._rows[:n, 0].cpu().numpy().view(U64)
            esc = (words & ESCAPE) != 0
            assert (raw[~esc] == U64(0xffffffffffffffff)).all()
        m = ws.matched[:n].cpu().numpy().view(U64)
        i = ws.ignored[:n].cpu().numpy().view(U64)
        assert not ws.rows_pending and ws.rows_expanded == int(compact)
        out.append((m, i, words))
    g_o, d_o = orclib.ranges(f)
    want_m, want_i, _, _ = orclib.match(f, g_o if gt_rng is None else gt_rng, d_o, detail=False)
    (m_c, i_c, words), (m_n, i_n, _) = out
    assert np.array_equal(m_n, want_m) and np.array_equal(i_n, want_i)
    assert np.array_equal(m_c, m_n) and np.array_equal(i_c, i_n)
    # a plain word is its row
    plain = (words & ESCAPE) == 0
    assert (words[~plain] == ESCAPE).all() and (words[plain] >> np.uint32(18) == 0).all()
    pm, pi = expand_products(words[plain])
    assert np.array_equal(pm, m_n[plain, 0]) and np.array_equal(pi, i_n[plain, 0])
    return words, m_n, i_n


@gpu
def test_compact_match_rows_of_the_long_category_problem(gathering):
    from test_gpu_sweep_modes import _long_category_problem
    _, _, f_l, _ = _long_category_problem()
    words, _, _ = _match_both_ways(gathering, f_l)
    assert 0 < int(((words & ESCAPE) != 0).sum()) < len(words) // 2


def _two_candidate_problem():
    """The cells of test_gpu_parity.py::test_cells_whose_detections_overlap_two_
    ground_truths: ground truths of a cell made near-duplicates of each other,
    detections jittered copies of them."""
    gt, dt = synth(seed=33, V=4, F=20, C=6, dets_per_frame=30, n_present=3)
    order = np.lexsort((gt.ann_cat, gt.ann_img))
    img, cat = gt.ann_img[order], gt.ann_cat[order]
    box = gt.ann_bbox.copy()
    same = np.flatnonzero((img[1:] == img[:-1]) & (cat[1:] == cat[:-1])) + 1
    assert len(same) > 50
    for k in same:
        box[order[k]] = box[order[k - 1]] + np.array([1.0, 2.0, 0.0, 1.0])
    gt.ann_bbox = box
    gt.ann_area = box[:, 2] * box[:, 3]
    rng = np.random.default_rng(5)
    key_g = gt.ann_img * 10 ** 6 + gt.ann_cat
    key_d = dt.image_id * 10 ** 6 + dt.category_id
    first = {}
    for j, k in enumerate(key_g.tolist()):
        first.setdefault(k, j)
    src = np.array([first.get(k, -1) for k in key_d.tolist()])
    has = src >= 0
    dbox = dt.bbox.copy()
    dbox[has] = box[src[has]] + rng.integers(-2, 3, (int(has.sum()), 4))
    dbox[:, 2:] = np.maximum(dbox[:, 2:], 1.0)
    dt.bbox = dbox
    return fl.flatten_lvis(gt, dt)


@gpu
def test_compact_match_rows_where_detections_overlap_two_ground_truths(gathering):
    words, _, _ = _match_both_ways(gathering, _two_candidate_problem())
    esc = int(((words & ESCAPE) != 0).sum())
    assert esc > 100 and esc < len(words)


def _mixed_runs_problem():
    """One category, one cell per image.  Images 1-3 form ONE run of the match
    plan that holds simple cells (1, 3) and a cell that goes through the greedy
    loop (2: near-duplicate ground truths); then runs of exactly 64 (simple),
    63 (greedy), 64 (simple), 1 (a NaN IoU: greedy) and 64 detections.  Image 3
    is not exhaustive for the category (unmatched detections are ignored) and
    holds the ground truth with the hidden id 0; ground truths ignored in every
    range (ignore flag), in some (visibility) and -- through the range table
    handed to the match -- in none; two detections do not consume their match."""
    cats = [{"id": 1, "name": "a", "frequency": "f"}]
    videos = [{"id": 10, "name": "v", "neg_category_ids": [],
               "not_exhaustive_category_ids": []}]
    images = [{"id": i, "video_id": 10, "frame_index": i, "neg_category_ids": [],
               "not_exhaustive_category_ids": [1] if i == 3 else []} for i in range(1, 9)]
    anns, preds, tracks = [], [], []

    def add_gt(img, box, vis=1.0, oof=False, ignore=False, ann_id=None, area=None):
        a = {"id": len(anns) + 1 if ann_id is None else ann_id, "image_id": img,
             "track_id": len(anns) + 1, "category_id": 1, "bbox": list(box),
             "area": box[2] * box[3] if area is None else area, "visibility": vis,
             "out_of_frame": oof}
        if ignore:
            a["ignore"] = 1
        tracks.append({"id": len(anns) + 1, "category_id": 1, "video_id": 10})
        anns.append(a)

    def add_dt(img, box):
        preds.append({"image_id": img, "category_id": 1, "bbox": list(box),
                      "score": 0.999 - 0.001 * len(preds), "track_id": len(preds) + 1,
                      "video_id": 10})

    rng = np.random.default_rng(12)

    def cloud(img, box, n):
        for _ in range(n):
            d = rng.integers(-12, 13, 4)
            add_dt(img, [box[0] + d[0], box[1] + d[1], max(box[2] + d[2], 1), max(box[3] + d[3], 1)])
    # image 1: simple -- one candidate each
    add_gt(1, [10, 10, 50, 50])
    add_gt(1, [200, 10, 50, 50], ignore=True)
    add_gt(1, [400, 10, 50, 50], vis=0.05)
    for b in ([10, 10, 50, 50], [12, 11, 50, 50], [201, 10, 50, 50], [400, 12, 50, 48],
              [700, 700, 20, 20]):
        add_dt(1, b)
    # image 2: greedy -- every detection overlaps both ground truths
    add_gt(2, [10, 10, 50, 50], vis=0.5)
    add_gt(2, [11, 12, 50, 51], vis=0.9, oof=True)
    for b in ([10, 10, 50, 50], [11, 11, 50, 50], [12, 12, 50, 50]):
        add_dt(2, b)
    # image 3: simple, not exhaustive, hidden id
    add_gt(3, [10, 10, 50, 50], ann_id=0)
    add_gt(3, [300, 10, 40, 40], vis=0.9, oof=True)
    for b in ([11, 10, 50, 50], [300, 11, 40, 40], [600, 600, 30, 30], [10, 12, 50, 49]):
        add_dt(3, b)
    # image 4: 64 detections, simple
    add_gt(4, [100, 100, 60, 60], vis=0.3)
    cloud(4, [100, 100, 60, 60], 64)
    # image 5: 63 detections, greedy
    add_gt(5, [100, 100, 60, 60])
    add_gt(5, [101, 102, 60, 61], vis=0.1)
    cloud(5, [100, 100, 60, 60], 63)
    # image 6: 64 detections on three separate ground truths, simple
    for x in (50, 300, 550):
        add_gt(6, [x, 50, 70, 70], vis=0.8)
    for k in range(64):
        cloud(6, [(50, 300, 550)[k % 3], 50, 70, 70], 1)
    # image 7: one detection, a ground truth whose width is a NaN
    add_gt(7, [20, 20, float("nan"), 40], area=1600.0)
    add_dt(7, [20, 20, 40, 40])
    # image 8: 64 detections
    add_gt(8, [30, 30, 80, 80], vis=0.95)
    cloud(8, [30, 30, 80, 80], 64)
    gtj = {"info": {}, "images": images, "videos": videos, "tracks": tracks,
           "annotations": anns, "categories": cats}
    f = fl.flatten_lvis(GTColumns.from_json(gtj), DTColumns.from_json(preds))
    # detections that do not consume their match: the first of image 1 (simple
    # path: the second one then matches the same ground truth) and of image 2
    flags = np.array(f.dt_flags)
    for c in (0, 1):
        flags[int(f.cell_dt_off[c])] |= fl.DT_NO_CONSUME
    f.dt_flags = flags
    return f


@gpu
def test_compact_match_rows_of_runs_that_mix_both_paths(gathering):
    engine = gathering
    f = _mixed_runs_problem()
    D = np.diff(f.cell_dt_off)
    assert D.tolist() == [5, 3, 4, 64, 63, 64, 1, 64]
    groups, singles = engine.match_plan(f.cell_dt_off, f.cell_gt_off)
    assert len(singles) == 0
    runs = [(int(a), int(b)) for a, b in groups]
    assert runs == [(0, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8)]
    assert (f.dt_flags & fl.DT_IGNORE_UNMATCHED).any() and (f.dt_flags & fl.DT_NO_CONSUME).any()
    assert (f.gt_flags & fl.GT_ID_HIDDEN).any()
    iou = orclib.run_flat(f)["iou"]
    assert np.isnan(iou).any()
    # range masks: every range (ignore flag), some, and -- set here -- none
    g_rng, _ = orclib.ranges(f)
    assert (g_rng == 0x3f).any() and ((g_rng != 0x3f) & (g_rng != 0)).any()
    g_rng = g_rng.copy()
    g_rng[int(f.cell_gt_off[5])] = 0              # a candidate of image 6
    words, m, i = _match_both_ways(engine, f, gt_rng=g_rng)
    esc = (words & ESCAPE) != 0
    off = f.cell_dt_off
    cell_esc = [bool(esc[off[c]:off[c + 1]].all()) for c in range(8)]
    cell_plain = [bool((~esc[off[c]:off[c + 1]]).all()) for c in range(8)]
    assert cell_esc == [False, True, False, False, True, False, True, False]
    assert cell_plain == [not e for e in cell_esc]
    # the fields show up in the words: unmatched-ignored and hidden in image 3,
    # an empty range mask in image 6, a full one in image 1
    w3 = words[off[2]:off[3]]
    assert ((w3 >> np.uint32(16)) & 1).all() and ((w3 >> np.uint32(17)) & 1).any()
    w6, w1 = words[off[5]:off[6]], words[off[0]:off[1]]
    assert (((w6 & 0x3ff) != 0) & (((w6 >> np.uint32(10)) & 63) == 0)).any()
    assert (((w1 & 0x3ff) != 0) & (((w1 >> np.uint32(10)) & 63) == 63)).any()
    # the detection that does not consume leaves its ground truth to the next one
    assert (words[0] & 0x3ff) and (words[1] & 0x3ff)


# ---------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------
SIZES = [0, 1, 511, 512, 513, 2047, 2048, 2049, 40 * SC + 17, 0, 700]
PATTERNS = ["none", "one_per_chunk", "first_and_last", "whole_chunk"]


def _escaped_places(pattern, sizes):
    """Sorted places whose rows are escaped, category by category (a chunk =
    512 consecutive sorted places of a category)."""
    esc = np.zeros(int(sum(sizes)), bool)
    rng = np.random.default_rng(41)
    at = 0
    for sz in sizes:
        for c0 in range(0, sz, CHUNK):
            c1 = min(c0 + CHUNK, sz)
            if pattern == "one_per_chunk":
                esc[at + c0 + int(rng.integers(0, c1 - c0))] = True
            elif pattern == "first_and_last":
                esc[at + c0] = esc[at + c1 - 1] = True
            elif pattern == "whole_chunk" and (c0 // CHUNK) % 3 == 1:
                esc[at + c0:at + c1] = True
        if pattern == "whole_chunk" and 0 < sz <= CHUNK:
            esc[at:at + sz] = True                        # (a partial chunk, whole)
        at += sz
    return esc


@functools.lru_cache(maxsize=None)
def _sweep_case(pattern):
    """Words in sorted order (m10 a run of thresholds, as the match produces, or
    any ten bits), rows = their expansion; an escaped place holds a row no word
    can say (random bits) and a word that would expand to something else."""
    rng = np.random.default_rng(7)
    sizes = SIZES
    K, n = len(sizes), int(sum(sizes))
    cat_off = np.zeros(K + 1, np.int32)
    np.cumsum(sizes, out=cat_off[1:])
    rank = np.concatenate([np.arange(s) / max(s, 1) for s in sizes]) if n else np.zeros(0)
    qpass = np.clip((rng.random(n) * 14 - 2 - 6 * rank).astype(np.int64), 0, 10)
    M = np.minimum(qpass, (rng.random(n) < 0.1) * rng.integers(0, 11, n))
    m10 = ((1 << qpass) - 1) & ~((1 << M) - 1)
    anyb = rng.random(n) < 0.1
    m10 = np.where(anyb, rng.integers(0, 1024, n), m10)
    g = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 64, n))
    u = rng.random(n) < 0.15
    h = rng.random(n) < 0.05
    words = (m10 | g << 10 | u.astype(np.int64) << 16 | h.astype(np.int64) << 17).astype(np.uint32)
    m, i = expand_products(words)
    esc = _escaped_places(pattern, sizes)
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
    from test_gpu_sweep_modes import _oracle_tables
    want_p, want_r = _oracle_tables(cat_off, matched, ignored, num_gt)
    order = np.arange(n, dtype=np.int32)          # shuffled inside the categories
    for a, b in zip(cat_off[:-1], cat_off[1:]):
        order[a:b] = a + rng.permutation(int(b - a))
    return cat_off, words, matched, ignored, num_gt, order, esc, want_p, want_r


def _compact_tables(case, hint, prepared):
    """taoamd_accumulate_by_order_compact: words and rows stored at order[p]; the
    row table holds the escaped rows and garbage everywhere else."""
    import torch
    lib = _lib.load()
    dev = "cuda:0"
    cat_off, words, matched, ignored, num_gt, order, esc, _, _ = case
    K, n_rng = num_gt.shape
    n = len(words)
    w_cell = np.empty_like(words)
    w_cell[order] = words
    rows = np.full((max(n, 1), 2), 0x6b6b6b6b6b6b6b6b, U64)
    rows[order[esc], 0] = matched[esc, 0]
    rows[order[esc], 1] = ignored[esc, 0]
    d_rows = torch.from_numpy(rows.view(np.int64)).to(dev)
    d_w = torch.from_numpy(w_cell.view(np.int32)).to(dev)
    d_off = torch.from_numpy(cat_off).to(dev)
    d_ng = torch.from_numpy(num_gt).to(dev)
    d_order = torch.from_numpy(order).to(dev)
    ws = wsguard.Guarded(lib.taoamd_accumulate_workspace(n, K, n_rng), dev)
    prec = torch.full((N_THR, N_REC, K, n_rng), 7.0, dtype=torch.float64, device=dev)
    rec = torch.full((N_THR, K, n_rng), 7.0, dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    if prepared:
        _lib.check(lib.taoamd_accumulate_prepare(n, K, n_rng, d_off.data_ptr(), hint,
                                                 ws.data_ptr(), ws.nbytes, s), "prepare")
    for _ in range(2 if prepared else 1):          # a prepared plan serves pass after pass
        _lib.check(lib.taoamd_accumulate_by_order_compact(
            n, K, n_rng, d_off.data_ptr(), d_order.data_ptr(), d_w.data_ptr(),
            d_rows.data_ptr(), d_ng.data_ptr(), hint, prec.data_ptr(), rec.data_ptr(),
            ws.data_ptr(), ws.nbytes, int(prepared), s), "by_order_compact")
    flag = C.c_int32(7)
    _lib.check(lib.taoamd_accumulate_error(ws.data_ptr(), s, C.addressof(flag)), "error")
    ws.check()
    return prec.cpu().numpy(), rec.cpu().numpy(), flag.value


@pytest.fixture(params=["lookback", "twopass"])
def onepass_mode(request):
    _lib.sweep_mode(request.param)
    yield request.param
    _lib.sweep_mode("auto")


@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
def test_compact_sweep_on_every_boundary_with_escaped_rows(onepass_mode, pattern):
    """Category lengths 0, 1, 511, 512, 513, 2047, 2048, 2049 and one of 40
    super-chunks; no escaped row, one per chunk, the first and the last row of
    every chunk, whole chunks (a partial one among them)."""
    case = _sweep_case(pattern)
    esc, want_p, want_r = case[6:]
    assert bool(esc.any()) == (pattern != "none")
    for hint, prepared in ((0, False), (int(max(SIZES)), False), (int(max(SIZES)), True)):
        got_p, got_r, flag = _compact_tables(case, hint, prepared)
        what = (onepass_mode, pattern, hint, prepared)
        assert flag == 0, what
        assert np.array_equal(got_r, want_r), what
        assert np.array_equal(got_p, want_p), what


@gpu
def test_compact_sweep_is_refused_where_another_kernel_would_run():
    """Under the chunked kernels (or the fused single-workgroup sweep) nobody
    reads the words: TAOAMD_ERR_ARG, not stale tables."""
    _lib.sweep_mode("chunked")
    try:
        with pytest.raises(_lib.TaoAmdError, match="bad argument"):
            _compact_tables(_sweep_case("none"), 0, False)
    finally:
        _lib.sweep_mode("auto")


# ---------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------
@gpu
def test_a_timed_out_compact_pass_is_expanded_and_swept_again(gathering, caplog):
    """engine.sweep_ok behind a compact pass whose look-backs all give up: the
    rows are expanded first, then swept by the chunked kernels through order[]."""
    import torch
    from test_gpu_sweep_modes import _long_category_problem
    engine = gathering
    _lib.sweep_mode("lookback", spin_limit=-1)
    _, _, f_l, _ = _long_category_problem()
    want = orclib.run_flat(f_l, detail=False)
    dp = engine.DeviceProblem(f_l, "cuda:0")
    ws = engine.Workspace(dp)
    assert ws.gather
    aux = torch.cuda.Stream("cuda:0")
    for rep in range(2):
        ws.precision.fill_(7.0)
        ws.rows.fill_(-1)
        engine.run_forked(dp, ws, aux)
        torch.cuda.synchronize()
        assert ws.cell_order and ws.rows_pending and ws.rows_expanded == rep
        assert engine.sweep_ok(dp, ws)
        assert ws.sweep_recovered == rep + 1
        assert not ws.rows_pending and ws.rows_expanded == rep + 1
        assert np.array_equal(ws.precision.cpu().numpy(), want["precision"])
        assert np.array_equal(ws.recall.cpu().numpy(), want["recall"])
    assert any("swept again" in r.getMessage() for r in caplog.records)


@gpu
def test_compact_and_scatter_passes_alternate_on_one_workspace(gathering):
    """The `aside` values of test_gpu_sweep_by_order's chain test: the views are
    expanded once after every compact pass, on the first read, and never stale."""
    import torch
    from test_gpu_sweep_modes import _long_category_problem
    engine = gathering
    _, _, f_l, _ = _long_category_problem()
    want = orclib.run_flat(f_l, detail=False)
    dp = engine.DeviceProblem(f_l, "cuda:0")
    ws = engine.Workspace(dp)
    assert ws.gather and ws.compact_buf is not None
    aux = torch.cuda.Stream("cuda:0")
    n = dp.n_dt
    expanded = 0
    for aside in (None, False, None, True):
        compact = aside is not False
        ws.precision.fill_(7.0)
        ws.rows.fill_(-1)                   # (a stale view would show this)
        assert ws.rows_expanded == expanded
        ws.compact_buf.fill_(0)
        engine.run_forked(dp, ws, aux, sort_aside=aside)
        torch.cuda.synchronize()
        assert ws.cell_order == compact and ws.rows_pending == compact
        assert not engine.sweep_ok(dp, ws)
        assert np.array_equal(ws.precision.cpu().numpy(), want["precision"]), aside
        assert np.array_equal(ws.recall.cpu().numpy(), want["recall"]), aside
        # the sweep did not need the rows: still unexpanded
        assert ws.rows_pending == compact and ws.rows_expanded == expanded
        if compact:
            plain = ws.compact_buf[:n] >= 0
            assert bool(plain.any()) and bool((~plain).any())
            assert bool((ws._rows[:n, 0, 0][plain] == -1).all())
        at = ws.dst[:n].long()
        assert np.array_equal(ws.matched[:n][at].cpu().numpy().view(U64), want["matched"]), aside
        expanded += int(compact)
        assert not ws.rows_pending and ws.rows_expanded == expanded
        assert np.array_equal(ws.ignored[:n][at].cpu().numpy().view(U64), want["ignored"]), aside
        assert torch.equal(ws.rows[:n, :, 0], ws.matched[:n])
        assert ws.rows_expanded == expanded                 # (cached until the next pass)
