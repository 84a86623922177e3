"""numpy restatement of the chunk format of csrc/exchange.hip (test
infrastructure: the gloo tests use it as the backend, the GPU tests compare
the HIP kernels with it byte for byte)."""
import numpy as np

# the score columns the exchange tests run on besides their own: any double
from scorepop import expected_order, score_population  # noqa: F401

N_THR, N_REC = 10, 101
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1,
                       endpoint=True)
# edited threshold sets: a shorter list padded with copies of its last value
# (what the class API hands the library), and one off the hundredths
PADDED_THRS = np.r_[np.linspace(0, 1, 11), np.ones(N_REC - 11)]
OFFGRID_THRS = np.linspace(0.005, 0.995, N_REC)


def align(x):
    return (x + 255) & ~255


def layout(block_cats, n_rng, capacity):
    rows = block_cats * n_rng
    hdr = align(rows * 8)          # num_gt[rows], off[rows]
    rec = align(rows * N_THR * 8)
    return hdr, rec, hdr + rec + align(capacity * 8)


# run_map: counts up to ARANGE_MAX take the reference's own expression, larger
# ones the windowed form (an arange of 2^31 doubles is 16 GB)
ARANGE_MAX = 20000
# Ground-truth counts at which a run map can go wrong.  Above 100 every column
# has a crossing of its own whatever the rounding (101 runs), so the rounding
# of c / ng against the threshold bit patterns decides the map only up to 100:
# 10 .. 90 are the counts a CPU search over 1 .. 20000 found to tell the wrong
# maps of test_exchange_ref_host.py from the true one besides 50 and 100.
COUNTS = (1, 2, 3, 49, 50, 51, 99, 100, 101, 102, 199, 200, 201, 1000, 12345,
          10 ** 6, 2 ** 31 - 2, 2 ** 31 - 1,
          10, 20, 25, 40, 75, 80, 90)
# candidates floor(x * ng) - WINDOW .. floor(x * ng) + WINDOW.  x * ng is off
# its real value by at most one rounding (relative 2^-53, far below 1 for
# ng < 2^31), and fl(c / ng) >= x can differ from c >= x * ng only where
# c / ng lies within a rounding of x, i.e. for the one or two integers next to
# x * ng: the answer lies in floor - 1 .. floor + 2.
# test_exchange_ref_host.py shows it never touches the window's edge.
WINDOW = 3
_MAPS = {}


def _thrs(rec_thrs):
    t = np.ascontiguousarray(rec_thrs, dtype=np.float64)
    assert t.shape == (N_REC,)
    return t


def crossings_arange(ng, rec_thrs=REC_THRS):
    """The reference's expression: first TP count whose recall reaches each
    threshold (lvis_amodal/eval.py:386,406)."""
    rc = np.arange(ng + 1, dtype=np.float64) / ng
    return np.searchsorted(rc, _thrs(rec_thrs), side="left")


def crossings_windowed(ng, rec_thrs=REC_THRS, with_base=False):
    """Per threshold x in [0, 1] the smallest c in the window around x * ng
    with c / ng >= x, in numpy doubles (c / ng is monotone in c, so the
    smallest c of the window is the smallest of all once c - 1 was tried)."""
    x = _thrs(rec_thrs)
    base = np.floor(x * np.float64(ng)).astype(np.int64)
    cand = base[:, None] + np.arange(-WINDOW, WINDOW + 1, dtype=np.int64)[None, :]
    ok = (cand >= 0) & (cand <= ng)
    with np.errstate(invalid="ignore"):
        ok &= cand.astype(np.float64) / np.float64(ng) >= x[:, None]
    assert ok.any(axis=1).all(), "no crossing inside the window"
    c = cand[np.arange(N_REC), ok.argmax(axis=1)]
    return (c, base) if with_base else c


def run_map(ng, rec_thrs=REC_THRS, crossings=None):
    """Run index of each recall column for a row with ng ground truths.
    `crossings`: the crossing function to use instead (not memoised)."""
    ng = int(ng)
    if crossings is None:
        key = (ng, _thrs(rec_thrs).tobytes())
        d = _MAPS.get(key)
        if d is not None:
            return d
        c = (crossings_arange if ng <= ARANGE_MAX else crossings_windowed)(ng, rec_thrs)
    else:
        c = crossings(ng, rec_thrs)
    d = np.zeros(N_REC, np.int64)
    d[1:] = np.cumsum(c[1:] != c[:-1])
    if crossings is None:
        d.setflags(write=False)
        _MAPS[key] = d
    return d


def sizes(block_cats, n_rng, world, num_gt, rec_thrs=REC_THRS):
    ng = np.asarray(num_gt).reshape(world, block_cats * n_rng)
    out = np.zeros(world, np.int64)
    for b in range(world):
        for n in ng[b]:
            if n > 0:
                out[b] += (run_map(int(n), rec_thrs)[-1] + 1) * N_THR
    return out


def _bits(a):
    """8-byte cells as uint64: the values travel as bit patterns (a record is
    often a NaN when read as a double)."""
    a = np.asarray(a)
    if a.dtype not in (np.uint64, np.int64):
        a = a.astype(np.float64, copy=False)
    return a.view(np.uint64)


def pack(n_cat, n_rng, block_cats, rank, num_gt, val, rec, capacity, rec_thrs=REC_THRS):
    """-> chunk bytes (uint8) of `rank`; tables addressed by global row."""
    hdr, recb, total = layout(block_cats, n_rng, capacity)
    rows = block_cats * n_rng
    chunk = np.zeros(total, np.uint8)
    h = chunk[:rows * 4].view(np.int32)
    ho = chunk[rows * 4:rows * 8].view(np.int32)
    r = chunk[hdr:hdr + rows * N_THR * 8].view(np.float64).reshape(rows, N_THR)
    lv = chunk[hdr + recb:hdr + recb + capacity * 8].view(np.uint64)
    ng = np.asarray(num_gt).reshape(-1)
    v = _bits(val).reshape(-1, N_THR, N_REC)
    rr = np.asarray(rec).reshape(-1, N_THR)
    off = 0
    r[:] = -1.0
    for i in range(rows):
        row = rank * rows + i
        n = int(ng[row]) if row < n_cat * n_rng else 0
        h[i] = n
        if n <= 0:
            continue
        r[i] = rr[row]
        ho[i] = off
        d = run_map(n, rec_thrs)
        first = np.r_[0, np.flatnonzero(d[1:] != d[:-1]) + 1]
        nd = len(first)
        lv[off:off + nd * N_THR] = v[row][:, first].reshape(-1)
        off += nd * N_THR
    return chunk


def decode_records(bits):
    """(tp << 32 | n) records of the device sweeps -> tp / (n + eps), the
    reference's precision expression (lvis_amodal/eval.py:384)."""
    bits = np.asarray(bits).view(np.uint64)
    tp = (bits >> np.uint64(32)).astype(np.float64)
    n = (bits & np.uint64(0xffffffff)).astype(np.float64)
    return tp / (n + np.spacing(1))


def unpack(n_cat, n_rng, block_cats, world, chunks, capacity, records=False,
           rec_thrs=REC_THRS):
    """records=True: the levels are the device sweeps' (tp, n) records."""
    hdr, recb, total = layout(block_cats, n_rng, capacity)
    rows = block_cats * n_rng
    chunks = np.asarray(chunks).view(np.uint8)
    KR = n_cat * n_rng
    precision = np.full((N_THR, N_REC, KR), -1.0)
    recall = np.full((N_THR, KR), -1.0)
    num_gt = np.zeros(KR, np.int32)
    for b in range(world):
        c = chunks[b * total:(b + 1) * total]
        h = c[:rows * 4].view(np.int32)
        ho = c[rows * 4:rows * 8].view(np.int32)
        r = c[hdr:hdr + rows * N_THR * 8].view(np.float64).reshape(rows, N_THR)
        lv = c[hdr + recb:hdr + recb + capacity * 8].view(np.float64)
        if records:
            lv = decode_records(lv)
        for i in range(rows):
            row = b * rows + i
            if row >= KR:
                break
            n = int(h[i])
            num_gt[row] = n
            recall[:, row] = r[i]
            if n <= 0:
                continue
            d = run_map(n, rec_thrs)
            nd = d[-1] + 1
            off = int(ho[i])
            block = lv[off:off + nd * N_THR].reshape(N_THR, nd)
            precision[:, :, row] = block[:, d]
    return (num_gt.reshape(n_cat, n_rng),
            precision.reshape(N_THR, N_REC, n_cat, n_rng),
            recall.reshape(N_THR, n_cat, n_rng))


def expand(n_cat, n_rng, num_gt, val, rec, records=True):
    """The result the exchange has to deliver, stated without the chunk format:
    precision[t, j, k, a] = the value of val[row, t, j], recall[t, k, a] =
    rec[row, t], -1 in both where the row has no ground truth."""
    KR = n_cat * n_rng
    ng = np.asarray(num_gt).reshape(KR)
    v = np.asarray(val).reshape(KR, N_THR, N_REC)
    v = decode_records(v) if records else v.astype(np.float64)
    live = ng > 0
    precision = np.where(live[None, None, :], v.transpose(1, 2, 0), -1.0)
    recall = np.where(live[None, :], np.asarray(rec).reshape(KR, N_THR).T, -1.0)
    return (precision.reshape(N_THR, N_REC, n_cat, n_rng),
            recall.reshape(N_THR, n_cat, n_rng))


# records every sweep can leave and a decoder can get wrong: value 0, the two
# values next to 1 (1 / (1 + eps) and 1), n and tp at the top of 32 bits
_SPECIAL = np.array([(0, 1), (1, 1), (2, 2), (7, 7), (0xffffffff, 0xffffffff),
                     (0, 0xffffffff), (1, 0xffffffff), (0xfffffffe, 0xffffffff),
                     (0x7ff00000, 0xfffffffe), (0x80000000, 0x80000000)], dtype=np.uint64)


def _draw_records(rng, shape):
    n = rng.integers(1, 1 << 32, size=shape, dtype=np.uint64)
    small = rng.random(shape) < 0.5
    n = np.where(small, n % np.uint64(50) + np.uint64(1), n)
    tp = (rng.random(shape) * (n.astype(np.float64) + 1)).astype(np.uint64)
    tp = np.minimum(tp, n)
    out = (tp << np.uint64(32)) | n
    sp = _SPECIAL[rng.integers(0, len(_SPECIAL), size=shape)]
    return np.where(rng.random(shape) < 0.25, (sp[..., 0] << np.uint64(32)) | sp[..., 1], out)


def count_rows(rows, counts=COUNTS):
    """num_gt of `rows` rows: the counts in turn at the even rows, zeros
    between them (every count appears once rows >= 2 * len(counts) - 1)."""
    ng = np.zeros(rows, np.int32)
    live = np.arange(0, rows, 2)
    ng[live] = np.asarray(counts, dtype=np.int64)[(live // 2) % len(counts)]
    return ng


def level_tables(num_gt, rng, rec_thrs=REC_THRS):
    """Valid inputs of the exchange for the rows' ground-truth counts:
    -> val [rows][N_THR][N_REC] (records, as float64 bit patterns) and rec
    [rows][N_THR].  The columns of one run of a row's map hold one record,
    as the sweep guarantees; neighbouring runs hold records of different
    VALUE, so a run boundary that moved shows in the chunk and in the
    expanded table.  Rows without ground truth hold garbage."""
    ng = np.asarray(num_gt).reshape(-1)
    rows = len(ng)
    # garbage: a record and a recall no live row can hold (live recalls lie in [0, 1))
    val = np.full((rows, N_THR, N_REC), (0xdead << 32) | 0xbeef, dtype=np.uint64)
    val[:, :, ::2] = 0xfff8000000000001
    rec = 1e300 + rng.random((rows, N_THR))
    for row in np.flatnonzero(ng > 0):
        d = run_map(int(ng[row]), rec_thrs)
        nd = int(d[-1]) + 1
        lv = _draw_records(rng, (N_THR, nd))
        while True:
            dv = decode_records(lv)
            same = np.zeros(lv.shape, bool)
            same[:, 1:] = dv[:, 1:] == dv[:, :-1]
            if not same.any():
                break
            lv[same] = _draw_records(rng, int(same.sum()))
        val[row] = lv[:, d]
        rec[row] = rng.random(N_THR)
    return val.view(np.float64), rec
