"""numpy restatement of track-level HOTA (the definition in
include/tao_amodal_hip.h, section "track-level HOTA"), in the same order of
operations.  TEST INFRASTRUCTURE ONLY.

The per-frame overlaps come from orclib.bb_iou; the sums of float terms run in
ascending row from 0.0 (never np.sum, which adds pairwise); everything that
crosses a frame is an integer in fixed point (ONE = 2^30).  The per-frame
assignment is identity_ref.hungarian on the compacted integer matrix: the
algorithm and the tie rule of the kernel, so its pairs are compared with ``==``.

hota_float() is a second, independent statement from the paper's formulas
(Luiten et al., IJCV 2021, and TrackEval's HOTA class) in plain float64 with
scipy.optimize.linear_sum_assignment."""
from types import SimpleNamespace

import numpy as np

import identity_ref
import orclib
from track_error_types_ref import make_track_flat

GT_IGNORE = 1
ONE = 1 << 30
EPS = np.finfo(float).eps
DEFAULT_ALPHAS = np.arange(0.05, 0.99, 0.05)
RATIOS = ("hota", "deta", "assa", "detre", "detpr", "assre", "asspr", "loca")


def cs(s):
    """c(s): 0 unless s > 0 (a NaN is 0), else min(s, 1)."""
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(s > 0, np.minimum(s, 1.0), 0.0)


def q(x):
    return np.rint(np.asarray(x, dtype=np.float64) * ONE).astype(np.int64)


def _kept(t, dt_keep):
    n_dt = int(np.asarray(t.cell_dt_off)[-1])
    return np.ones(n_dt, bool) if dt_keep is None else np.asarray(dt_keep)[:n_dt] != 0


def _eligible(t):
    n_gt = int(np.asarray(t.cell_gt_off)[-1])
    return (np.asarray(t.gt_flags)[:n_gt] & GT_IGNORE) == 0


def frame_groups(t, dt_keep=None, bb_iou=None):
    """Every frame group with a ground truth, cells and positions ascending:
    (cell, p, gl, gf, dl, df, S) -- the in-cell rows and the frame indices of Gp
    and Dp in ascending row, S float64[|Dp|, |Gp|] the overlaps."""
    bb_iou = bb_iou or orclib.bb_iou
    d_off, g_off = np.asarray(t.cell_dt_off, np.int64), np.asarray(t.cell_gt_off, np.int64)
    dfoff, gfoff = np.asarray(t.dt_frame_off, np.int64), np.asarray(t.gt_frame_off, np.int64)
    dfpos, gfpos = np.asarray(t.dt_frame_pos, np.int64), np.asarray(t.gt_frame_pos, np.int64)
    dfbox = np.asarray(t.dt_frame_box, dtype=np.float64).reshape(-1, 4)
    gfbox = np.asarray(t.gt_frame_box, dtype=np.float64).reshape(-1, 4)
    kept, elig = _kept(t, dt_keep), _eligible(t)

    def side(r0, r1, on, foff, fpos):
        rows = [r for r in range(r0, r1) if on[r]]
        fr = np.concatenate([np.arange(foff[r], foff[r + 1]) for r in rows] +
                            [np.zeros(0, np.int64)]).astype(np.int64)
        own = np.concatenate([np.full(foff[r + 1] - foff[r], r - r0) for r in rows] +
                             [np.zeros(0, np.int64)]).astype(np.int64)
        by = np.argsort(fpos[fr], kind="stable")       # (a position's rows stay ascending)
        return fpos[fr][by], fr[by], own[by]
    for c in range(len(d_off) - 1):
        g_pos, g_fr, g_own = side(g_off[c], g_off[c + 1], elig, gfoff, gfpos)
        d_pos, d_fr, d_own = side(d_off[c], d_off[c + 1], kept, dfoff, dfpos)
        for p in np.unique(g_pos):
            a, b = np.searchsorted(g_pos, p, "left"), np.searchsorted(g_pos, p, "right")
            x, y = np.searchsorted(d_pos, p, "left"), np.searchsorted(d_pos, p, "right")
            gl, gf, dl, df = g_own[a:b], g_fr[a:b], d_own[x:y], d_fr[x:y]
            if len(df):
                with np.errstate(all="ignore"):
                    S = np.asarray(bb_iou(dfbox[df], gfbox[gf]), np.float64).reshape(len(df), len(gf))
            else:
                S = np.zeros((0, len(gf)))
            yield c, int(p), gl, gf, dl, df, S


def align(t, dt_keep=None, bb_iou=None):
    """pot int64[n_iou]."""
    ioff = np.asarray(t.cell_iou_off, np.int64)
    G = np.diff(np.asarray(t.cell_gt_off, np.int64))
    pot = np.zeros(int(ioff[-1]), np.int64)
    for c, _, gl, _, dl, _, S in frame_groups(t, dt_keep, bb_iou):
        if not len(dl):
            continue
        C = cs(S)
        rowsum, colsum = np.zeros(len(gl)), np.zeros(len(dl))
        for j in range(len(dl)):
            rowsum = rowsum + C[j]
        for i in range(len(gl)):
            colsum = colsum + C[:, i]
        den = (rowsum[None, :] + colsum[:, None]) - C
        with np.errstate(all="ignore"):
            a = np.where(den > 2.0 ** -52, np.minimum(C / den, 1.0), 0.0)
        a = np.where(C > 0, a, 0.0)
        pot[ioff[c] + dl[:, None] * G[c] + gl[None, :]] += q(a)
    return pot


def gas_of(pot, L, F):
    """The global alignment score of pot[..] for the frame counts L, F."""
    pot = np.asarray(pot, np.int64)
    P = pot.astype(np.float64) / ONE
    with np.errstate(all="ignore"):
        g = P / ((L + F).astype(np.float64) - P)
        g = np.where(g > 0, np.minimum(g, 1.0), 0.0)
    return np.where(pot > 0, g, 0.0)


def match(t, pot, alphas, dt_keep=None, bb_iou=None):
    """dict(mc int32[A, n_iou], lc int64[A, n_iou], match int32[n_gt_frames],
    match_iou, groups): groups = [(cell, p, gf, dl, W int64[|Gp|, |Dp|], pairs,
    gl)] with pairs = [(i, j)], the places in Gp and Dp of the assigned pairs."""
    alphas = np.asarray(alphas, np.float64)
    ioff = np.asarray(t.cell_iou_off, np.int64)
    d_off, g_off = np.asarray(t.cell_dt_off, np.int64), np.asarray(t.cell_gt_off, np.int64)
    G = np.diff(g_off)
    L = np.diff(np.asarray(t.gt_frame_off, np.int64))
    F = np.diff(np.asarray(t.dt_frame_off, np.int64))
    n_iou, n_gf = int(ioff[-1]), len(np.asarray(t.gt_frame_pos))
    pot = np.asarray(pot, np.int64)
    mc, lc = np.zeros((len(alphas), n_iou), np.int32), np.zeros((len(alphas), n_iou), np.int64)
    mt, mi = -np.ones(n_gf, np.int32), np.zeros(n_gf)
    groups = []
    for c, p, gl, gf, dl, df, S in frame_groups(t, dt_keep, bb_iou):
        if not len(dl):
            groups.append((c, p, gf, dl, np.zeros((len(gl), 0), np.int64), [], gl))
            continue
        word = ioff[c] + dl[None, :] * G[c] + gl[:, None]            # [|Gp|, |Dp|]
        C = cs(S).T
        gas = gas_of(pot[word], L[g_off[c] + gl][:, None], F[d_off[c] + dl][None, :])
        W = np.where(C > 0, q(gas * C), 0)
        rows, cols = np.flatnonzero(W.max(1) > 0), np.flatnonzero(W.max(0) > 0)
        pairs = []
        if len(rows) and len(cols):
            # (hungarian takes the smaller side as rows, the first when equal)
            _, asg = identity_ref.hungarian(W[np.ix_(rows, cols)])
            pairs = [(int(rows[r]), int(cols[j])) for r, j in enumerate(asg)
                     if j >= 0 and W[rows[r], cols[j]] > 0]
        for i, j in pairs:
            mt[gf[i]], mi[gf[i]] = dl[j], S[j, i]
            on = alphas <= C[i, j]
            mc[on, word[i, j]] += 1
            lc[on, word[i, j]] += q(C[i, j])
        groups.append((c, p, gf, dl, W, pairs, gl))
    return dict(mc=mc, lc=lc, match=mt, match_iou=mi, groups=groups)


def term(m, den):
    """q'(m * min(m / den, 1)); 0 where den is not positive."""
    m, den = np.asarray(m, np.float64), np.asarray(den, np.float64)
    with np.errstate(all="ignore"):
        r = np.where(den > 0, np.minimum(m / den, 1.0), 0.0)
    return q(m * r)


def reduce(t, mc, lc, n_cat):
    """(tp int64[K, A], loc int64[K, A], ass int64[K, A, 3])."""
    mc, lc = np.asarray(mc, np.int64), np.asarray(lc, np.int64)
    A = mc.shape[0]
    ioff = np.asarray(t.cell_iou_off, np.int64)
    d_off, g_off = np.asarray(t.cell_dt_off, np.int64), np.asarray(t.cell_gt_off, np.int64)
    L = np.diff(np.asarray(t.gt_frame_off, np.int64))
    F = np.diff(np.asarray(t.dt_frame_off, np.int64))
    elig, gt_cat = _eligible(t), np.asarray(t.gt_cat, np.int64)
    tp, loc = np.zeros((n_cat, A), np.int64), np.zeros((n_cat, A), np.int64)
    ass = np.zeros((n_cat, A, 3), np.int64)
    for c in range(len(d_off) - 1):
        D, G = d_off[c + 1] - d_off[c], g_off[c + 1] - g_off[c]
        if not D or not G:
            continue
        m = mc[:, ioff[c]:ioff[c] + D * G].reshape(A, D, G)
        l = lc[:, ioff[c]:ioff[c] + D * G].reshape(A, D, G)
        Fd = F[d_off[c]:d_off[c + 1]][None, :, None].astype(np.float64)
        for g in range(G):
            row = g_off[c] + g
            if not elig[row] or not 0 <= gt_cat[row] < n_cat:
                continue
            mg = np.where(m[:, :, g:g + 1] > 0, m[:, :, g:g + 1], 0)
            on = mg > 0
            k = gt_cat[row]
            tp[k] += mg.sum((1, 2))
            loc[k] += np.where(on, l[:, :, g:g + 1], 0).sum((1, 2))
            Lg = float(L[row])
            for col, den in enumerate(((Lg + Fd) - mg, Lg + 0 * Fd, Fd + 0.0 * mg)):
                ass[k, :, col] += np.where(on, term(mg, den), 0).sum((1, 2))
    return tp, loc, ass


def stage(t, alphas, dt_keep=None, n_cat=None, bb_iou=None):
    """All three calls: dict(pot, mc, lc, match, match_iou, groups, tp, loc, ass)."""
    n_cat = len(t.cat_ids) if n_cat is None else n_cat
    pot = align(t, dt_keep, bb_iou)
    out = match(t, pot, alphas, dt_keep, bb_iou)
    out["pot"] = pot
    out["tp"], out["loc"], out["ass"] = reduce(t, out["mc"], out["lc"], n_cat)
    return out


def frame_counts(t, dt_keep=None, n_cat=None):
    """int64[K, 4] = gt_tracks, gt_frames, dt_tracks, dt_frames over the eligible
    and the kept tracks: the identity's first four cat_counts columns."""
    n_cat = len(t.cat_ids) if n_cat is None else n_cat
    out = np.zeros((n_cat, 4), np.int64)
    L = np.diff(np.asarray(t.gt_frame_off, np.int64))
    F = np.diff(np.asarray(t.dt_frame_off, np.int64))
    for g in np.flatnonzero(_eligible(t)):
        if 0 <= t.gt_cat[g] < n_cat:
            out[t.gt_cat[g], :2] += [1, L[g]]
    for d in np.flatnonzero(_kept(t, dt_keep)):
        if 0 <= t.dt_cat[d] < n_cat:
            out[t.dt_cat[d], 2:] += [1, F[d]]
    return out


def ratios(tp, loc, ass, gt_frames, dt_frames):
    """The class layer's arithmetic: dict of the eight float64 arrays in the shape
    of tp, from integer tables; gt_frames and dt_frames broadcast against tp."""
    tp = np.asarray(tp, np.int64)
    fn, fp = np.asarray(gt_frames, np.int64) - tp, np.asarray(dt_frames, np.int64) - tp
    tpf = tp.astype(np.float64)
    one = np.maximum(1, tp).astype(np.float64)
    ass = np.asarray(ass, np.int64).astype(np.float64) / ONE
    out = {"deta": tpf / np.maximum(1, tp + fn + fp), "detre": tpf / np.maximum(1, tp + fn),
           "detpr": tpf / np.maximum(1, tp + fp), "assa": ass[..., 0] / one,
           "assre": ass[..., 1] / one, "asspr": ass[..., 2] / one}
    with np.errstate(all="ignore"):
        out["loca"] = np.where(tp > 0, np.asarray(loc, np.int64).astype(np.float64) / ONE / one,
                               1.0)
    out["hota"] = np.sqrt(out["deta"] * out["assa"])
    return out


def hota_float(t, alphas, dt_keep=None, n_cat=None):
    """The paper's formulas in plain float64, scipy's assignment: dict of the
    eight ratios float64[K, A], "tp" int64[K, A] and "pairs": {(cell, p): the
    sorted (in-cell d, in-cell g) of the frame's assignment with a score > 0}."""
    from scipy.optimize import linear_sum_assignment
    n_cat = len(t.cat_ids) if n_cat is None else n_cat
    alphas = np.asarray(alphas, np.float64)
    A = len(alphas)
    d_off, g_off = np.asarray(t.cell_dt_off, np.int64), np.asarray(t.cell_gt_off, np.int64)
    L = np.diff(np.asarray(t.gt_frame_off, np.int64)).astype(np.float64)
    F = np.diff(np.asarray(t.dt_frame_off, np.int64)).astype(np.float64)
    cnt = frame_counts(t, dt_keep, n_cat)
    frames = list(frame_groups(t, dt_keep))
    pmc = {}
    for c, _, gl, _, dl, _, S in frames:
        sim = cs(S).T                                            # [g, d]
        den = sim.sum(0)[None, :] + sim.sum(1)[:, None] - sim
        iou = np.zeros_like(sim)
        ok = den > 0 + EPS
        iou[ok] = sim[ok] / den[ok]
        m = pmc.setdefault(c, np.zeros((g_off[c + 1] - g_off[c], d_off[c + 1] - d_off[c])))
        m[np.ix_(gl, dl)] += iou
    tp, loc = np.zeros((n_cat, A)), np.zeros((n_cat, A))
    ass = np.zeros((n_cat, A, 3))
    counts, pairs = {}, {}
    for c, p, gl, _, dl, _, S in frames:
        Lg, Fd = L[g_off[c]:g_off[c + 1]][:, None], F[d_off[c]:d_off[c + 1]][None, :]
        gas = pmc[c] / (Lg + Fd - pmc[c])
        sim = cs(S).T
        score = gas[np.ix_(gl, dl)] * sim
        rows, cols = linear_sum_assignment(-score)
        on = score[rows, cols] > 0
        rows, cols = rows[on], cols[on]
        pairs[(c, p)] = sorted(zip(dl[cols].tolist(), gl[rows].tolist()))
        m = counts.setdefault(c, np.zeros((A,) + pmc[c].shape))
        k = int(t.gt_cat[g_off[c]])
        for a, alpha in enumerate(alphas):
            hit = sim[rows, cols] >= alpha
            m[a, gl[rows[hit]], dl[cols[hit]]] += 1
            if 0 <= k < n_cat:
                loc[k, a] += sim[rows[hit], cols[hit]].sum()
    for c, m in counts.items():
        k = int(t.gt_cat[g_off[c]])
        if not 0 <= k < n_cat:
            continue
        Lg, Fd = L[g_off[c]:g_off[c + 1]][None, :, None], F[d_off[c]:d_off[c + 1]][None, None, :]
        tp[k] += m.sum((1, 2))
        ass[k, :, 0] += (m * (m / np.maximum(1, Lg + Fd - m))).sum((1, 2))
        ass[k, :, 1] += (m * (m / np.maximum(1, Lg + 0 * Fd))).sum((1, 2))
        ass[k, :, 2] += (m * (m / np.maximum(1, Fd + 0 * Lg))).sum((1, 2))
    fn, fp = cnt[:, 1:2] - tp, cnt[:, 3:4] - tp
    one = np.maximum(1, tp)
    out = {"deta": tp / np.maximum(1, tp + fn + fp), "detre": tp / np.maximum(1, tp + fn),
           "detpr": tp / np.maximum(1, tp + fp), "assa": ass[..., 0] / one,
           "assre": ass[..., 1] / one, "asspr": ass[..., 2] / one,
           "loca": np.where(tp > 0, loc / one, 1.0)}
    out["hota"] = np.sqrt(out["deta"] * out["assa"])
    out["tp"], out["pairs"] = tp.astype(np.int64), pairs
    return out


def fixed_pairs(want):
    """{(cell, p): sorted (in-cell d, in-cell g)} of match()'s groups."""
    out = {}
    for c, p, _, dl, _, pr, gl in want["groups"]:
        out[(c, p)] = sorted((int(dl[j]), int(gl[i])) for i, j in pr)
    return out


# ---------------------------------------------------------------------------
# seeded populations
# ---------------------------------------------------------------------------
def seeded_flat(seed, cells, lengths, timeline=160, n_cat=3, boxes=None, real=False):
    """A video per entry of cells = [(detection tracks, ground truths)], its cell
    of category v % n_cat.  Ground-truth tracks of `lengths` frames with holes on
    the timeline; about two thirds of the detection tracks are drifting copies of
    parts of a ground truth of their cell, a tenth lies behind the timeline.
    Integer boxes that move by pixels; real=True: boxes of any real size and
    place (no two weights equal); boxes(n): n pairs of any double (boxpop)."""
    rng = np.random.default_rng(seed)

    def positions():
        n = int(rng.choice(lengths))
        span = min(timeline, n + int(rng.integers(0, n // 4 + 2)))
        lo = int(rng.integers(0, timeline - span + 1)) if span < timeline else 0
        return np.sort(lo + rng.choice(span, min(n, span), replace=False))

    def box():
        if real:
            return (rng.random(4) * [20, 20, 10, 10] + [0, 0, 6, 6]).tolist()
        return [int(v) for v in (*rng.integers(0, 4, 2) * 3, *rng.choice([6, 8, 12], 2))]

    def drift(b):
        if real:
            return (np.asarray(b) + rng.normal(0, 0.8, 4) * [1, 1, 0.3, 0.3]).tolist()
        return [b[0] + int(rng.integers(-1, 2)), b[1] + int(rng.integers(0, 2)), b[2], b[3]]
    dets, gts = [], []
    for v, (nd, ng) in enumerate(cells):
        cat = v % n_cat
        mine = []
        for _ in range(ng):
            pos = positions()
            if boxes is None:
                b = box()
                fr = {int(p): drift(b) for p in pos}
                pop = None
            else:
                pop = boxes(len(pos))
                fr = {int(p): pop[2 * k + 1].tolist() for k, p in enumerate(pos)}
            mine.append((pos, fr, pop))
            gts.append((v, cat, fr, int(rng.choice([0, 0, 0, 1]))))
        for _ in range(nd):
            r = rng.random()
            pos, fr = positions(), None
            if r < 0.1:
                pos = np.unique(timeline + pos % 40)
            if ng and r >= 0.33:
                gpos, gfr, gpop = mine[int(rng.integers(ng))]
                keep = rng.random(len(gpos)) < rng.choice([0.4, 0.7, 1.0])
                keep = keep if keep.any() else np.ones(len(gpos), bool)
                pos = gpos[keep]
                if boxes is None:
                    fr = {int(p): drift(gfr[int(p)]) for p in pos}
                else:
                    fr = {int(p): gpop[2 * k].tolist() for k, p in zip(np.flatnonzero(keep), pos)}
            if fr is None:
                if boxes is None:
                    b = box()
                    fr = {int(p): drift(b) for p in pos}
                else:
                    pop = boxes(len(pos))
                    fr = {int(p): pop[2 * k].tolist() for k, p in enumerate(pos)}
            dets.append((v, cat, fr, float(rng.integers(0, 20)) / 20, 0))
    f, _, _ = make_track_flat(len(cells), n_cat, dets, gts)
    return f


def one_frame_table(shapes, rng, n_cat=3):
    """A cell per (|Gp|, |Dp|) of `shapes` whose tracks all have ONE frame at
    position 0: the cell is one frame group.  Boxes [0, 0, 10, h] with h in 1 ..
    10, so that c(s) = min(h) / max(h) takes many values, 1 among them."""
    G = np.array([s[0] for s in shapes], np.int64)
    D = np.array([s[1] for s in shapes], np.int64)
    n_gt, n_dt = int(G.sum()), int(D.sum())
    t = SimpleNamespace(n_cells=len(shapes), cat_ids=np.arange(n_cat, dtype=np.int64))
    t.cell_dt_off = np.r_[0, np.cumsum(D)].astype(np.int32)
    t.cell_gt_off = np.r_[0, np.cumsum(G)].astype(np.int32)
    t.cell_iou_off = np.r_[0, np.cumsum(D * G)].astype(np.int64)
    t.gt_cat = np.repeat(np.arange(len(shapes)) % n_cat, G).astype(np.int32)
    t.dt_cat = np.repeat(np.arange(len(shapes)) % n_cat, D).astype(np.int32)
    t.gt_flags = np.zeros(n_gt, np.uint8)
    t.dt_frame_off = np.arange(n_dt + 1, dtype=np.int32)
    t.gt_frame_off = np.arange(n_gt + 1, dtype=np.int32)
    t.dt_frame_pos, t.gt_frame_pos = np.zeros(n_dt, np.int32), np.zeros(n_gt, np.int32)

    def boxes(n):
        b = np.zeros((n, 4))
        b[:, 2], b[:, 3] = 10, rng.integers(1, 11, n)
        return b
    t.dt_frame_box, t.gt_frame_box = boxes(n_dt), boxes(n_gt)
    return t


# ---------------------------------------------------------------------------
# The hand-written table, two categories; alphas = HAND_ALPHAS unless said.
# ---------------------------------------------------------------------------
BOX = [0, 0, 10, 10]
HALF = [0, 0, 10, 5]          # IoU with BOX: 50 / (100 + 50 - 50) = 0.5 exactly
AWAY = [100, 100, 10, 10]     # 0 with BOX
HAND_ALPHAS = DEFAULT_ALPHAS - EPS
HAND_GTS = [
    # video 0, category 0: the paper's example -- one ground truth of 4 frames
    (0, 0, {p: BOX for p in range(4)}, 0),                               # 0
    # video 1, category 1: one frame where greedy by s and the optimum differ.
    # c = [[2/3, 7/13], [1/2, 0]] for [C, D] x [1, 2]: greedy takes (C, 1) and is left
    # with (D, 2) = 0; w = [[.162, .155], [.136, 0]] gives (C, 2) + (D, 1)
    (1, 1, {0: BOX}, 0),                                                 # 1
    (1, 1, {0: [0, 5, 10, 10]}, 0),                                      # 2
    # video 2, category 1: an eligible and an ignored ground truth
    (2, 1, {0: BOX, 1: BOX}, 0),                                         # 3
    (2, 1, {p: AWAY for p in range(3)}, GT_IGNORE),                      # 4
    # video 4, category 1 on the cell tables, a category outside the table in gt_cat
    (4, 1, {0: BOX, 1: BOX}, 0),                                         # 5
]
HAND_DETS = [
    (0, 0, {0: BOX, 1: BOX}, 0.9, 0),                                    # 0  A
    (0, 0, {2: BOX, 3: BOX}, 0.8, 0),                                    # 1  B
    (1, 1, {0: [0, 2, 10, 10]}, 0.9, 0),                                 # 2  C
    (1, 1, {0: HALF}, 0.8, 0),                                           # 3  D
    # E overlaps ground truth 3 at exactly 0.5 on frame 0
    (2, 1, {0: HALF, 1: BOX}, 0.7, 0),                                   # 4  E
    # F would win both frames: it is set aside (dt_keep = 0), as is H on the ignored one
    (2, 1, {0: BOX, 1: BOX}, 0.9, 0),                                    # 5  F
    (2, 1, {p: AWAY for p in range(3)}, 0.8, 0),                         # 6  H
    # video 3: a cell without ground truth, three frames of false positives
    (3, 1, {p: BOX for p in range(3)}, 0.9, 0),                          # 7  I
    (4, 1, {0: BOX, 1: BOX}, 0.9, 0),                                    # 8  J
]
A_, B_, C_, D_, E_, F_, H_, I_, J_ = range(9)
HAND_SET_ASIDE = [F_, H_]
# per ground-truth frame in the order given: the detection given or -1, and s
HAND_MATCH = [A_, A_, B_, B_, D_, C_, E_, E_, -1, -1, -1, J_, J_]
HAND_MATCH_IOU = [1, 1, 1, 1, 0.5, 7 / 13, 0.5, 1, 0, 0, 0, 1, 1]
# alphas 0.05 .. 0.50 (ten) and 0.55 .. 0.95 (nine)
HAND_TP = [[4] * 19, [4] * 10 + [1] * 9]
# category 0: ground truth 0 (4 frames), A and B (2 + 2); category 1: ground truths
# 1, 2, 3 (1 + 1 + 2), C, D, E, I kept (1 + 1 + 2 + 3)
HAND_COUNTS = [[1, 4, 2, 4], [3, 4, 4, 7]]
# category 0: (A, 0) and (B, 0) with m = 2, L = 4, F = 2: 2 * 2 / (4 + 2 - 2) = 1 each
# category 1, low alphas: (D, 1), (C, 2) with m = L = F = 1 and (E, 3) with m = L = F = 2:
# 1 + 1 + 2; high alphas: (E, 3) with m = 1: 1 / (2 + 2 - 1)
HAND_ASS0 = [[2 * ONE] * 19, [4 * ONE] * 10 + [357913941] * 9]
HAND_DETA = [[1.0] * 19, [4 / 7] * 10 + [1 / 10] * 9]
HAND_ASSA = [[0.5] * 19, [1.0] * 10 + [357913941 / ONE] * 9]
HAND_HOTA0 = 0.5 ** 0.5
# alphas = [0.5]: the pairs at exactly 0.5 count; [0.5 + 2^-52]: they do not
HAND_TP_AT_HALF = [[4], [4]]
HAND_TP_ABOVE_HALF = [[4], [2]]


def hand_flat():
    """(flat, dt_at, gt_at, dt_keep)."""
    f, dt_at, gt_at = make_track_flat(5, 2, HAND_DETS, HAND_GTS)
    f.gt_cat = np.array(f.gt_cat)
    f.dt_cat = np.array(f.dt_cat)
    f.gt_cat[gt_at[5]] = 7
    f.dt_cat[dt_at[J_]] = 7
    keep = np.ones(len(HAND_DETS), np.uint8)
    keep[dt_at[HAND_SET_ASIDE]] = 0
    return f, dt_at, gt_at, keep


def match_by_given(t, dt_at, gt_at, match_rows):
    """match int32[n_gt_frames] as the numbers of the detections given, per
    ground-truth frame in the order the ground truths were given."""
    d_inv = {int(r): i for i, r in enumerate(dt_at)}
    out = []
    gfoff, d_off = np.asarray(t.gt_frame_off), np.asarray(t.cell_dt_off)
    for g in gt_at:
        for k in range(gfoff[g], gfoff[g + 1]):
            m = int(match_rows[k])
            out.append(d_inv[int(d_off[t.gt_cell[g]]) + m] if m >= 0 else -1)
    return out
