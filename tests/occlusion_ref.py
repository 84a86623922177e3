"""numpy restatement of the track-level occlusion episodes (the definition in
include/tao_amodal_hip.h, section "track-level occlusion episodes").  TEST
INFRASTRUCTURE ONLY.  Everything is an integer: every comparison against the
device is ``==``."""
import numpy as np

GT_IGNORE = 1
START, UNFOLLOWED, END, KEPT, SWITCHED, LOST = range(6)
OUTCOMES = ("START", "UNFOLLOWED", "END", "KEPT", "SWITCHED", "LOST")
EPISODE_COLUMNS = ("gt", "a", "n", "outcome", "entry", "after", "gap", "covered", "held")
TRACK_COLUMNS = ("episodes", "frames", "kept", "switched_lost")
COUNT_COLUMNS = ("episodes", "frames", "covered", "held", "start", "unfollowed", "end",
                 "kept", "switched", "lost", "gap")


def track_episodes(best, vis, lo, hi, recover):
    """The episodes of one track as rows (a, n, outcome, entry, after, gap,
    covered, held); best int[L], vis float[L]."""
    best, vis = [int(b) for b in best], np.asarray(vis, dtype=np.float64)
    L = len(best)
    with np.errstate(invalid="ignore"):
        occ = ((lo <= vis) & (vis <= hi)).tolist()       # (a NaN compares false)
    out, k = [], 0
    while k < L:
        if not occ[k]:
            k += 1
            continue
        a = k
        while k + 1 < L and occ[k + 1]:
            k += 1
        b, k = k, k + 1
        entry = best[a - 1] if a > 0 else -1
        covered = sum(1 for x in best[a:b + 1] if x >= 0)
        held = sum(1 for x in best[a:b + 1] if x == entry) if entry >= 0 else 0
        after, gap = -1, 0
        for r in range(1, recover + 1):
            if b + r <= L - 1 and best[b + r] >= 0:
                after, gap = best[b + r], r - 1
                break
        if a == 0:
            outcome = START
        elif entry < 0:
            outcome = UNFOLLOWED
        elif b == L - 1:
            outcome = END
        elif after == entry:
            outcome = KEPT
        elif after >= 0:
            outcome = SWITCHED
        else:
            outcome = LOST
        if outcome in (START, UNFOLLOWED, END):
            after, gap = -1, 0
        out.append((a, b - a + 1, outcome, entry, after, gap, covered, held))
    return out


def occlusions(frame_off, vis, best, gt_cat, gt_flags, n_cat, lo, hi, recover, len_edges):
    """dict(episodes int32[n_ep, 9], gt_occ int32[n_gt, 4], counts int64[n_cat,
    n_len, 11], ep_off int64[n_gt + 1]) of the tracks whose frames are
    frame_off[g] .. frame_off[g + 1]."""
    edges = [int(x) for x in len_edges]
    assert 1 <= recover <= 64 and 1 <= len(edges) <= 8 and edges[0] == 1
    assert all(a < b for a, b in zip(edges, edges[1:])) and lo <= hi
    n_gt = len(frame_off) - 1
    episodes, gt_occ = [], np.zeros((n_gt, 4), np.int32)
    counts = np.zeros((n_cat, len(edges), 11), np.int64)
    ep_off = np.zeros(n_gt + 1, np.int64)
    for g in range(n_gt):
        s, e = int(frame_off[g]), int(frame_off[g + 1])
        eps = track_episodes(best[s:e], vis[s:e], lo, hi, recover)
        ep_off[g + 1] = ep_off[g] + len(eps)
        for a, n, outcome, entry, after, gap, covered, held in eps:
            episodes.append((g, a, n, outcome, entry, after, gap, covered, held))
            gt_occ[g] += [1, n, outcome == KEPT, outcome in (SWITCHED, LOST)]
            if gt_flags[g] & GT_IGNORE:
                continue
            j = max(i for i, x in enumerate(edges) if x <= n)
            row = [1, n, covered, held] + [int(outcome == o) for o in range(6)] + [gap]
            counts[gt_cat[g], j] += row
    return dict(episodes=np.asarray(episodes, np.int32).reshape(-1, 9), gt_occ=gt_occ,
                counts=counts, ep_off=ep_off)


def pack(tracks):
    """(frame_off int32[n + 1], vis float64[F], best int32[F], gt_cat int32[n],
    gt_flags uint8[n]) from tracks given as (category, flags, best list, vis list)."""
    off = np.zeros(len(tracks) + 1, np.int32)
    off[1:] = np.cumsum([len(t[2]) for t in tracks])
    assert all(len(t[2]) == len(t[3]) for t in tracks)
    vis = np.asarray([v for t in tracks for v in t[3]], dtype=np.float64)
    best = np.asarray([b for t in tracks for b in t[2]], dtype=np.int32)
    return (off, vis, best, np.asarray([t[0] for t in tracks], np.int32),
            np.asarray([t[1] for t in tracks], np.uint8))


# ---------------------------------------------------------------------------
# The hand-written table: window [0, 0.1], len_edges (1, 2, 3), two categories.
# ---------------------------------------------------------------------------
NAN = float("nan")
HAND_WINDOW = (0.0, 0.1)
HAND_EDGES = (1, 2, 3)
HAND_TRACKS = [
    # 0: the worked example of the definition
    (0, 0, [0, 0, -1, 0, 0, 1, 1, -1, -1, 0], [1, .1, 0, 1, .05, .05, 1, 0, 1, 1]),
    # 1: occluded throughout: START, not END
    (0, 0, [2, 2, -1], [0, 0, .1]),
    # 2: ends occluded: END
    (1, 0, [3, 3, -1, 3], [1, 1, 0, 0]),
    # 3: a NaN splits a run; nothing covered behind the second one
    (1, 0, [1, 1, 1, 1, -1], [1, 0, NAN, 0, 1]),
    # 4: "ignore": in the records, in no count
    (0, GT_IGNORE, [0, -1, 0], [1, 0, 1]),
    # 5: nobody follows on entry
    (1, 0, [-1, 0, 0], [1, 0, 1]),
    # 6: a track without frames
    (0, 0, [], []),
]
# (track, a, n, outcome, entry, after, gap, covered, held) at recover >= 2
HAND_EPISODES = [
    (0, 1, 2, KEPT, 0, 0, 0, 1, 1),
    (0, 4, 2, SWITCHED, 0, 1, 0, 2, 1),
    (0, 7, 1, SWITCHED, 1, 0, 1, 0, 0),
    (1, 0, 3, START, -1, -1, 0, 2, 0),
    (2, 2, 2, END, 3, -1, 0, 1, 1),
    (3, 1, 1, KEPT, 1, 1, 0, 1, 1),
    (3, 3, 1, LOST, 1, -1, 0, 1, 1),
    (4, 1, 1, KEPT, 0, 0, 0, 0, 0),
    (5, 1, 1, UNFOLLOWED, -1, -1, 0, 1, 0),
]
# at recover = 1 the third episode finds nobody behind it
HAND_EPISODE2_RECOVER1 = (0, 7, 1, LOST, 1, -1, 0, 0, 0)
HAND_GT_OCC = [[3, 5, 1, 2], [1, 3, 0, 0], [1, 2, 0, 0], [2, 2, 1, 1], [1, 1, 1, 0],
               [1, 1, 0, 0], [0, 0, 0, 0]]
HAND_GT_OCC0_RECOVER1 = [3, 5, 1, 2]
HAND_EP_OFF = [0, 3, 4, 5, 7, 8, 9, 9]
# [category][bucket]: episodes, frames, covered, held, start, unfollowed, end, kept,
# switched, lost, gap; track 4 is in none
HAND_COUNTS = [
    [[1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 1], [2, 4, 3, 2, 0, 0, 0, 1, 1, 0, 0],
     [1, 3, 2, 0, 1, 0, 0, 0, 0, 0, 0]],
    [[3, 3, 3, 2, 0, 1, 0, 1, 0, 1, 0], [1, 2, 1, 1, 0, 0, 1, 0, 0, 0, 0], [0] * 11],
]
HAND_COUNTS00_RECOVER1 = [1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0]
# occlusion_lines() of the table: the totals over both categories
HAND_LINES = [
    " track occlusions @[ frame IoU=0.50 | vis=[0, 0.1] | recover=2 ]",
    " length  episodes     kept% switched%     lost%     held%",
    " 1              4     33.33     33.33     33.33     50.00",
    " 2              3     50.00     50.00      0.00     50.00",
    " 3+             1         -         -         -      0.00",
]
# a visibility exactly at lo and exactly at hi is occluded, the doubles next to them
# are not: window [0.05, 0.1]
EDGE_WINDOW = (0.05, 0.1)
EDGE_TRACK = (0, 0, [0] * 6, [np.nextafter(0.05, 0), 0.05, 0.1, np.nextafter(0.1, 1), 0.1, 1])
EDGE_EPISODES = [(0, 1, 2, KEPT, 0, 0, 0, 2, 2), (0, 4, 1, KEPT, 0, 0, 0, 1, 1)]


def hand(recover=2, tracks=HAND_TRACKS, window=HAND_WINDOW, edges=HAND_EDGES, n_cat=2):
    """(packed tables, restatement) of the hand-written table."""
    t = pack(tracks)
    return t, occlusions(t[0], t[1], t[2], t[3], t[4], n_cat, window[0], window[1], recover, edges)
