"""Run-length masks at every edge of the mask IoU kernels: the seeded
population the run-length tests share (test_rle_domain_host.py,
test_gpu_rle_domain.py, golden/make_golden_maskapi.py).  A sibling of
boxpop.py: pure numpy, no GPU.

A mask is the oracle's dict {"h", "w", "counts"} (oracle/rle.py).  Within a
pair both masks have one frame size and sum(counts) == h * w < 2^32; only the
deliberate other-size masks of the cells differ.  Every kind returns
(items, claims): its pairs (d, g) -- cells and track problems for the last two
kinds -- and a dict of what it claims to contain, which the host test checks.

The kernels' edges (csrc/rle_walk.hpp, rle_iou.hip, track_mask_iou.hip): a
lane keeps RPT = 8 consecutive run boundaries of the detection, a wavefront
PIECE = 512 of them at a time; a lane follows the ground truth's runs for 4
steps, then bisects; 64 ground truths per tile; an LDS table of 6144 runs; 8
wavefronts per cell; 64 frames per ballot, 4 track pairs per block."""
import numpy as np

PAIR_KINDS = ("pieces", "dense", "ties", "empty_runs", "big_frames")
H, W = 64, 90
N = H * W
PIECE, FOLLOW, GTILE, LDS_RUNS = 512, 4, 64, 6144
KA = (1, 2, 3, 7, 8, 9, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 1537)
KB = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025)
TWO31, TWO32 = 1 << 31, 1 << 32
_SEEDS = {k: 20261019 + i for i, k in enumerate(PAIR_KINDS + ("cells", "tracks"))}


def mask(h, w, counts):
    return {"h": int(h), "w": int(w), "counts": [int(c) for c in counts]}


def from_ends(n, ends, lead=False):
    """Runs that end at the sorted pixels `ends` (< n) and at n; `lead` puts an
    empty run of zeros in front (the mask starts with ones)."""
    runs = np.diff(np.r_[0, np.asarray(ends, dtype=np.int64), n]).tolist()
    return ([0] + runs) if lead else runs


def k_runs(rng, n, k, lead=False):
    """A list of exactly k runs, all but an optional leading one non-empty."""
    m = k - 1 if lead else k
    if lead and k == 1:
        return [n]
    ends = np.sort(rng.choice(np.arange(1, n), size=m - 1, replace=False))
    return from_ends(n, ends, lead)


def splice(counts, at):
    """[0, 0] behind run `at`: the same pixels, two empty runs."""
    return list(counts[:at + 1]) + [0, 0] + list(counts[at + 1:])


# ------------------------------------------------- what the reference counts
def stop_pixel(a, b):
    """First pixel that the reference's loops (rleIou, rleMerge) do not count
    on run lists a, b of one total; the total when they count all.  They stop
    when the pixels left in the two current runs add up to 0 as C uints: where
    both masks finish a run and go on with an empty one, or where the two
    current runs have 2^32 pixels left between them (looked at whenever a
    cursor has just taken a new run)."""
    n = int(sum(a))
    ea, eb = np.cumsum(a, dtype=np.int64), np.cumsum(b, dtype=np.int64)

    def halts(c, e):
        return {int(e[i]) for i in range(len(c) - 1)
                if c[i + 1] == 0 and (c[i] > 0 or i == 0)}
    stops = [p for p in halts(a, ea) & halts(b, eb) if p < n]
    ev = np.unique(np.r_[ea, eb, 0 if (a[0] == 0 or b[0] == 0) else ea[0]])
    ev = ev[ev < n]
    left = lambda e: e[np.searchsorted(e, ev, side="right")] - ev
    stops += ev[left(ea) + left(eb) == TWO32].tolist()
    return min(stops) if stops else n


def count_before(a, b, p):
    """(|A & B|, |A | B|) over the pixels [0, p), by sorting the run ends."""
    ea, eb = np.cumsum(a, dtype=np.int64), np.cumsum(b, dtype=np.int64)
    cut = np.unique(np.minimum(np.r_[0, ea, eb, p], p))
    lo, n = cut[:-1], np.diff(cut)
    va = np.searchsorted(ea, lo, side="right") & 1      # the run a segment lies in
    vb = np.searchsorted(eb, lo, side="right") & 1
    return int(n[(va & vb) == 1].sum()), int(n[(va | vb) == 1].sum())


def predicted(d, g):
    """(i, u) of a pair of one frame size by the stop rule."""
    return count_before(d["counts"], g["counts"], stop_pixel(d["counts"], g["counts"]))


def most_between(a, b):
    """Most run ends of b behind one run end of a and up to the next: above
    FOLLOW the lane that holds them has to bisect."""
    ea, eb = np.cumsum(a, dtype=np.int64), np.cumsum(b, dtype=np.int64)
    return int(np.diff(np.searchsorted(eb, ea, side="right")).max()) if len(ea) > 1 else 0


def has_empty(c):
    return any(x == 0 for x in c[1:])


def _pair(h, w, a, b):
    assert sum(a) == sum(b) == h * w < TWO32
    return mask(h, w, a), mask(h, w, b)


# -------------------------------------------------------------------- kinds
def pieces():
    rng = np.random.default_rng(_SEEDS["pieces"])
    combos = [(ka, kb) for ka in KA for kb in (3, 65, 1025)] + \
             [(ka, kb) for kb in KB for ka in (2, 17, 1537)]
    pairs = [_pair(H, W, k_runs(rng, N, ka, lead=bool(i & 1) and ka > 1),
                   k_runs(rng, N, kb, lead=bool(i & 2) and kb > 1))
             for i, (ka, kb) in enumerate(combos)]
    return pairs, dict(n=len(combos), multi_piece=sum(ka > PIECE for ka, _ in combos),
                       ka=set(KA), kb=set(KB), lead_a=sum(p[0]["counts"][0] == 0 for p in pairs),
                       lead_b=sum(p[1]["counts"][0] == 0 for p in pairs))


def dense():
    """2000 three-pixel runs of one mask inside one run of the other."""
    h, w = 100, 200
    n, m, s = h * w, 2000, 400
    stretch = s + 3 * np.arange(m + 1)                   # B's ends: s, s + 3, ...
    pairs = []
    for j in range(6):
        x = int(stretch[m - j])                          # B's stretch ends j runs behind x
        for lead in (False, True):
            a = from_ends(n, [100, x, n - 50], lead)
            pairs.append(_pair(h, w, a, from_ends(n, stretch)))
            pairs.append(_pair(h, w, from_ends(n, stretch, lead), a))      # the reverse
    b = from_ends(n, stretch)
    pairs.append(_pair(h, w, [100, n - 100], b))         # A's last boundary = the frame's end
    pairs.append(_pair(h, w, [0, n], b))
    pairs.append(_pair(h, w, from_ends(n, [50, 55, n - 60, n - 55]), b))   # two distant parts
    pairs.append(_pair(h, w, from_ends(n, [50, 55, n - 60]), b))           # ... the last to the end
    return pairs, dict(n=len(pairs), bisect=len(pairs) - 12, follow_0_to_5=12)


def ties():
    rng = np.random.default_rng(_SEEDS["ties"])
    pool = np.sort(rng.choice(np.arange(1, N), size=60, replace=False))
    pairs = []
    for i in range(24):
        ca = pool[rng.random(60) < 0.6]
        cb = pool[rng.random(60) < 0.6]
        pairs.append(_pair(H, W, from_ends(N, ca, bool(i & 1)), from_ends(N, cb, bool(i & 2))))
    for lead in (False, True):
        a = from_ends(N, pool[::2], lead)
        pairs.append(_pair(H, W, a, list(a)))                              # identical
        pairs.append(_pair(H, W, a, from_ends(N, pool[::2], not lead)))    # complements
        pairs.append(_pair(H, W, a, from_ends(N, pool[::2] + 1, lead)))    # moved by a pixel
        pairs.append(_pair(H, W, a, from_ends(N, pool[::2] - 1, lead)))
    return pairs, dict(n=len(pairs), identical=2, complements=2, shifted=4)


TABLE_ROWS = (([2, 0, 0, 4], [2, 0, 0, 4]), ([2, 0, 0, 4], [2, 4]),
              ([1, 2, 0, 0, 3], [3, 0, 0, 3]))


def empty_runs():
    rng = np.random.default_rng(_SEEDS["empty_runs"])
    pool = np.sort(rng.choice(np.arange(200, N - 200), size=30, replace=False))
    both = pool[::3]                                      # ends that A and B share
    a0 = from_ends(N, np.sort(np.r_[both, pool[1::3]]))
    b0 = from_ends(N, np.sort(np.r_[both, pool[2::3]]), lead=True)
    at = lambda c, p: int(np.flatnonzero(np.cumsum(c) == p)[0])      # the run that ends at p
    own_a, own_b = int(pool[1]), int(pool[2])
    pairs, stop_at = [], []

    def add(a, b, p=None, h=H, w=W):
        pairs.append(_pair(h, w, a, b))
        stop_at.append(p)
    add(splice(a0, at(a0, own_a)), b0)                                # A only
    add(a0, splice(b0, at(b0, own_b)))                                # B only
    add(splice(a0, at(a0, own_a)), splice(b0, at(b0, own_b)))         # both, apart
    add(splice(a0, at(a0, int(both[1]))), splice(b0, at(b0, int(both[2]))))   # ... at shared ends
    for p in (int(both[0]), int(both[len(both) // 2]), int(both[-1])):
        add(splice(a0, at(a0, p)), splice(b0, at(b0, p)), p)         # first / middle / last
    add([0, 0] + a0, [0, 0] + b0[1:], 0)                              # at pixel 0
    add([0, 0] + a0, b0)                                              # ... on one side only
    add(a0 + [0, 0], b0 + [0, 0])                                     # trailing: stops nothing
    p1, p2 = int(both[3]), int(both[6])
    add(splice(splice(a0, at(a0, p2)), at(a0, p1)),
        splice(splice(b0, at(b0, p2)), at(b0, p1)), p1)               # two stops: the first
    add(splice(a0, at(a0, p1)) + [0, 0, 0], splice(b0, at(b0, p1)) + [0], p1)
    long_a = k_runs(rng, N, 700)                                      # a stop in the second piece
    p = int(np.cumsum(long_a)[600])
    long_b = from_ends(N, [37, p, N - 11])
    add(splice(long_a, 600), splice(long_b, 1), p)
    add(splice(long_b, 1), splice(long_a, 600), p)
    # a stop before any pixel is shared: i = 0, the IoU is 0 over a union of 1
    add(splice([100, 50, N - 150], 1), splice([150, N - 150], 0), 150)
    add([100, 50, 0, 0, 10, N - 160], [150, 0, 0, 10, N - 160], 150)
    for a, b in TABLE_ROWS:
        add(a, b, 2 if b == [2, 0, 0, 4] else 3 if len(a) == 5 else None, 2, 3)
    return pairs, dict(n=len(pairs), stop_at=stop_at,
                       stopped=sum(p is not None for p in stop_at))


BIG = ((1, TWO31 - 1), (32768, 65536), (65535, 65537), (2, (1 << 30) + 3))
PER_BIG = 15                    # pairs per frame size


def literal(d, g):
    """Whether the kernels walk the pair with the reference's two cursors (a
    superset of the pairs that stop early) and not by prefix sums."""
    return has_empty(g["counts"]) or max(d["counts"]) + max(g["counts"]) >= TWO32


def big_frames():
    rng = np.random.default_rng(_SEEDS["big_frames"])
    pairs = []
    for h, w in BIG:
        n = h * w
        full, half, thin = [0, n], [n // 2, n - n // 2], [5, 3, n - 8]
        late = [n - n // 4, n // 4]
        many = [from_ends(n, np.sort(rng.choice(np.unique(rng.integers(1, n, size=640)),
                                                size=599, replace=False)), lead)
                for lead in (False, True)]
        dots = []                                   # ones with 300 single zeros in them
        for _ in range(2):
            z = np.unique(rng.integers(1, n - 2, size=300) & ~1)
            dots.append(from_ends(n, np.sort(np.r_[z, z + 1]), lead=True))
        most = [n // 8, n - n // 8]
        for a, b in ((dots[0], dots[1]), (dots[1], most), (most, dots[0]), (full, full), (full, half), (half, full), (half, half), (thin, full),
                     (full, thin), (late, half), (half, late), ([1, n - 1], full),
                     (many[0], many[1]), (many[1], half), (full, many[0])):
            pairs.append(_pair(h, w, a, list(b)))
    return pairs, dict(n=len(pairs), frames=[h * w for h, w in BIG])


def pairs_of(kind):
    return {"pieces": pieces, "dense": dense, "ties": ties, "empty_runs": empty_runs,
            "big_frames": big_frames}[kind]()


# -------------------------------------------------------------------- cells
def cells():
    """Cells of taoamd_rle_iou: (dts, gts) lists of masks.  A ground-truth
    tile holds mostly masks that are settled without a walk -- empty ones (no
    box: 0) and full ones of another frame size (-1) -- and walked ones on
    chosen lanes."""
    rng = np.random.default_rng(_SEEDS["cells"])
    src = {k: pairs_of(k)[0] for k in PAIR_KINDS}
    small = [p for p in src["pieces"]
             if 2 <= len(p[0]["counts"]) <= 17 and 2 <= len(p[1]["counts"]) <= 129]
    long_ = [p for p in src["pieces"] if len(p[0]["counts"]) == 513 and len(p[1]["counts"]) == 65]
    mixed = small + src["ties"][:8] + [p for p in src["empty_runs"] if p[0]["h"] == H] + long_
    out, walked_lanes = [], set()

    def cell(D, G, pool, lanes):
        picks = [pool[int(i)] for i in rng.choice(len(pool), size=max(D, len(lanes)))]
        h, w = picks[0][0]["h"], picks[0][0]["w"]
        dts = [picks[i % len(picks)][0] for i in range(D)]
        gts = [mask(h, w, [h * w]) if j % 3 else mask(h + 1, w, [0, (h + 1) * w])
               for j in range(G)]
        for n, j in enumerate(lanes):
            if j < G:
                gts[j] = picks[n % len(picks)][1]
                walked_lanes.add(j)
        out.append((dts, gts))
    shapes = [(1, 1), (7, 63), (8, 64), (9, 65), (17, 128), (1, 129), (9, 129), (8, 1)]
    for n, (D, G) in enumerate(shapes):
        cell(D, G, mixed, (0, 5, 62, 63, 64, 70, 127, 128))
        if n % 2 == 0:
            out.append(([], [mask(H, W, [N])] * 3) if n % 4 == 0 else ([mask(H, W, [N])] * 2, []))
    cell(1, 65, src["dense"], (0, 63, 64))
    cell(2, 65, src["big_frames"][PER_BIG:2 * PER_BIG], (0, 63, 64))
    for extra in (143, 144, 145):                   # the LDS table's edge
        gts = [mask(H, W, k_runs(rng, N, 1000, lead=bool(j & 1))) for j in range(6)]
        gts.append(mask(H, W, k_runs(rng, N, extra)))
        out.append(([mask(H, W, k_runs(rng, N, 40)), src["empty_runs"][4][0]], gts))
    out.append(([], []))
    return out, dict(n=len(out), G={len(g) for _, g in out}, D={len(d) for d, _ in out},
                     walked_lanes=walked_lanes,
                     gt_runs={sum(len(m["counts"]) for m in g) for _, g in out})


# ------------------------------------------------------------------- tracks
def column_edges():
    """h = 1, so a pixel is a column: spans that share exactly one column and
    spans that are adjacent, for an odd and an even number of runs per side."""
    w = 40
    rows = [([10, 10, 20], [19, 6, 15], 1), ([10, 10, 20], [20, 5, 15], 0),
            ([30, 5, 5], [34, 6], 1), ([30, 5, 5], [35, 5], 0),
            ([30, 10], [25, 6, 9], 1), ([30, 10], [25, 5, 10], 0),
            ([30, 10], [39, 1], 1), ([34, 6], [30, 5, 5], 1), ([35, 5], [30, 5, 5], 0)]
    return [_pair(1, w, a, b) for a, b, _ in rows], [s for _, _, s in rows]


def frame_pool():
    """Pairs of frame masks for the track problems."""
    src = {k: pairs_of(k)[0] for k in PAIR_KINDS}
    pool = [p for p in src["pieces"] if len(p[0]["counts"]) + len(p[1]["counts"]) <= 150][:12]
    pool += [p for p in src["pieces"] if len(p[0]["counts"]) == 513][:1]
    big = src["big_frames"]
    pool += src["ties"][:6] + src["empty_runs"]
    pool += big[:6] + big[PER_BIG:PER_BIG + 6] + big[2 * PER_BIG:2 * PER_BIG + 4]
    pool += column_edges()[0]
    # the first / the last run of ones is empty, on either side
    odd = [[5, 0, 10, 3, N - 18], [5, 3, 10, 0, N - 18], [5, 3, N - 8, 0], [0, 0, 7, 4, N - 11]]
    pool += [_pair(H, W, a, [4, 9, N - 13]) for a in odd[:3]]
    pool += [_pair(H, W, odd[3], [7, 4, N - 11])]
    pool += [_pair(H, W, [4, 9, N - 13], a) for a in odd[:3]]
    return pool


def tracks():
    """Problems of taoamd_track_mask_iou with 3, 4 and 5 track pairs: each a
    list of cells (dt tracks, gt tracks), a track a dict {position: mask}.
    The detection's mask on position t is the d of pool[t % len(pool)]; a
    ground-truth track with offset o carries the g of pool[(t + o) % len]
    (o = 0: the d's own partner)."""
    pool = frame_pool()
    L = len(pool)
    dt = lambda pos: {int(t): pool[t % L][0] for t in pos}
    gt = lambda pos, o=0: {int(t): pool[(t + o) % L][1] for t in pos}
    r = lambda n, s=0: range(s, s + n)
    p3 = [([dt(r(63))], [gt(r(63)), gt(r(40, 200)), gt([62, 63, 64])])]
    p4 = [([dt(r(64)), dt(r(65))], [gt([0, 63, 64, 90]), gt(r(65), 1)])]
    p5 = [([dt(r(129))], [gt(r(129)), gt([63, 64, 127, 128, 129])]),
          ([dt(r(5)), dt(r(3))], []),
          ([dt(range(0, 258, 2))], [gt(r(129), 3), gt(range(1, 259, 2)), gt([64 * 2, 128 * 2])]),
          ([], [])]
    probs = [p3, p4, p5]
    return probs, dict(pairs=[sum(len(d) * len(g) for d, g in p) for p in probs],
                       dt_frames={len(t) for p in probs for d, _ in p for t in d},
                       pool=L)
