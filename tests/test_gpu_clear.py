"""-m gpu: track-level CLEAR (taoamd_track_clear_count, _fill, _walk, _reduce,
engine.stage_track_clear, TaoEval.clear) against the numpy restatement of
tests/clear_ref.py.  Every call goes through the ABI with a workspace of exactly
the reported size behind a guard band and with outputs pre-filled with junk;
every device output is an integer (cand_iou, match_iou: one box_iou value) and is
compared with ==.  The per-step assignment is checked for validity and against
scipy's optimum on the integer matrix as well."""
from types import SimpleNamespace

import numpy as np
import pytest

import association_ref
import boxpop
import clear_ref as ref
import hota_ref
import identity_ref
import orclib
import wsguard
from goldenio import path
from tao_amodal_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ONE = ref.ONE
STORE = ("cand_off", "cand_row", "cand_q", "cand_iou", "step")
WALKED = ("match", "match_iou", "sw", "gt_clear")


def _up(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], dtype=dtype)
    return torch.from_numpy(a).to(DEV)


def _junk(shape, dtype, fill):
    import torch
    return torch.full(shape, fill, dtype=dtype, device=DEV)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _sizes(t):
    """n_dt, n_gt, n_cells, n_dt_frames, n_gt_frames."""
    return (int(t.cell_dt_off[-1]), int(t.cell_gt_off[-1]), len(t.cell_dt_off) - 1,
            len(getattr(t, "dt_frame_pos", ())), len(t.gt_frame_pos))


def _ws(sizes):
    lib = _lib.load()
    return wsguard.Guarded(lib.taoamd_track_clear_workspace(sizes[0], sizes[1], sizes[4]), DEV)


def _cand_tables(t, keep):
    cols = [_up(t.cell_dt_off, np.int32), _up(t.cell_gt_off, np.int32), _up(t.gt_flags, np.uint8),
            _up(keep, np.uint8) if keep is not None else None,
            _up(t.dt_frame_off, np.int32), _up(t.dt_frame_pos, np.int32),
            _up(np.asarray(t.dt_frame_box, dtype=np.float64).reshape(-1, 4), np.float64),
            _up(t.gt_frame_off, np.int32), _up(t.gt_frame_pos, np.int32),
            _up(np.asarray(t.gt_frame_box, dtype=np.float64).reshape(-1, 4), np.float64)]
    return cols, [c.data_ptr() if c is not None else None for c in cols]


def _device_candidates(t, thr, keep=None, fill=-3, with_iou=True):
    import torch
    lib, sizes = _lib.load(), _sizes(t)
    n_gf = sizes[4]
    hold, ptrs = _cand_tables(t, keep)
    off = _junk((n_gf + 1,), torch.int64, fill)
    step = _junk((max(n_gf, 1),), torch.uint8, fill & 0xff)
    ws = _ws(sizes)
    _lib.check(lib.taoamd_track_clear_count(
        *sizes, thr, *ptrs, off.data_ptr(), step.data_ptr(), ws.data_ptr(), ws.nbytes, _stream()),
        "taoamd_track_clear_count")
    ws.check()
    n = int(off[-1].item())
    row = _junk((max(n, 1),), torch.int32, fill)
    q = _junk((max(n, 1),), torch.int32, fill)
    iou = _junk((max(n, 1),), torch.float64, float(fill))
    ws = _ws(sizes)
    _lib.check(lib.taoamd_track_clear_fill(
        *sizes, thr, *ptrs, off.data_ptr(), n, row.data_ptr(), q.data_ptr(),
        iou.data_ptr() if with_iou else None, ws.data_ptr(), ws.nbytes, _stream()),
        "taoamd_track_clear_fill")
    ws.check()
    return dict(cand_off=off.cpu().numpy(), cand_row=row[:n].cpu().numpy(),
                cand_q=q[:n].cpu().numpy(), cand_iou=iou[:n].cpu().numpy(),
                step=step[:n_gf].cpu().numpy())


def _store_ptrs(c, hold, with_iou=True):
    hold.extend([_up(c["cand_off"], np.int64), _up(c["cand_row"], np.int32),
                 _up(c["cand_q"], np.int32),
                 _up(c["cand_iou"], np.float64) if with_iou and c.get("cand_iou") is not None
                 else None])
    return [h.data_ptr() if h is not None else None for h in hold[-4:]]


def _device_walk(t, c, fill=-3, with_iou=True):
    import torch
    lib, sizes, hold = _lib.load(), _sizes(t), []
    n_dt, n_gt, n_cells, _, n_gf = sizes
    n_cand = len(c["cand_row"])
    cols = [_up(t.cell_dt_off, np.int32), _up(t.cell_gt_off, np.int32), _up(t.gt_flags, np.uint8),
            _up(t.gt_frame_off, np.int32), _up(t.gt_frame_pos, np.int32)]
    store = _store_ptrs(c, hold, with_iou)
    step = _up(c["step"], np.uint8)
    mt = _junk((max(n_gf, 1),), torch.int32, fill)
    mi = _junk((max(n_gf, 1),), torch.float64, float(fill))
    sw = _junk((max(n_gf, 1),), torch.uint8, fill & 0xff)
    gc = _junk((max(n_gt, 1), 4), torch.int32, fill)
    status = _junk((1,), torch.int32, fill)
    ws = _ws(sizes)
    _lib.check(lib.taoamd_track_clear_walk(
        n_dt, n_gt, n_cells, n_gf, n_cand, *[x.data_ptr() for x in cols], *store,
        step.data_ptr(), mt.data_ptr(), mi.data_ptr() if with_iou else None, sw.data_ptr(),
        gc.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.nbytes, _stream()),
        "taoamd_track_clear_walk")
    ws.check()
    return dict(match=mt[:n_gf].cpu().numpy(), match_iou=mi[:n_gf].cpu().numpy(),
                sw=sw[:n_gf].cpu().numpy(), gt_clear=gc[:n_gt].cpu().numpy(),
                status=int(status.item()))


def _device_reduce(t, c, match, sw, gt_clear, vis=None, vis_rng=None, n_cat=None, fill=-3):
    import torch
    lib, sizes, hold = _lib.load(), _sizes(t), []
    n_dt, n_gt, _, _, n_gf = sizes
    n_cat = len(t.cat_ids) if n_cat is None else n_cat
    rng = np.asarray(vis_rng if vis_rng is not None else [], np.float64).reshape(-1, 2)
    n_vis = len(rng)
    cols = [_up(t.gt_cat, np.int32), _up(t.gt_flags, np.uint8), _up(t.gt_frame_off, np.int32)]
    visd = _up(vis, np.float64) if n_vis else None
    rngd = _up(rng, np.float64) if n_vis else None
    store = _store_ptrs(c, hold)[:3]
    outs = [_up(match, np.int32), _up(sw, np.uint8), _up(np.asarray(gt_clear).reshape(-1, 4),
                                                         np.int32)]
    cc = _junk((n_cat, 7), torch.int64, fill)
    vc = _junk((max(n_vis, 1), n_cat, 4), torch.int64, fill)
    ws = _ws(sizes)
    _lib.check(lib.taoamd_track_clear_reduce(
        n_dt, n_gt, n_gf, len(c["cand_row"]), n_cat, n_vis, *[x.data_ptr() for x in cols],
        visd.data_ptr() if n_vis else None, rngd.data_ptr() if n_vis else None, *store,
        *[x.data_ptr() for x in outs], cc.data_ptr(), vc.data_ptr() if n_vis else None,
        ws.data_ptr(), ws.nbytes, _stream()), "taoamd_track_clear_reduce")
    ws.check()
    return cc.cpu().numpy(), vc[:n_vis].cpu().numpy()


def _device_stage(t, thr, keep=None, vis=None, vis_rng=None, n_cat=None, fill=-3):
    out = _device_candidates(t, thr, keep, fill)
    out.update(_device_walk(t, out, fill))
    out["cat_counts"], out["vis_counts"] = _device_reduce(
        t, out, out["match"], out["sw"], out["gt_clear"], vis, vis_rng, n_cat, fill)
    return out


def _same(got, want, keys):
    for k in keys:
        assert got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k], want[k]), k
    assert got.get("status", 0) == 0


def _check_steps(t, got, want):
    """Per step the device's pairs are a valid one-to-one set of candidates whose
    weights, with the bonus computed from the DEVICE's own previous step, add up
    to scipy's optimum on that integer matrix."""
    from scipy.optimize import linear_sum_assignment
    frame_gt = np.repeat(np.arange(len(t.gt_frame_off) - 1), np.diff(t.gt_frame_off))
    last = {}                                                # g -> (stepno, d) on the device
    for cell, _, gf, cols, W, prevs, _, stepno in want["steps"]:
        cols = np.asarray(cols)
        base = np.where(W >= ref.BONUS, W - ref.BONUS, W)    # (every q <= ONE < BONUS)
        prev = np.array([last.get(frame_gt[k], (-9, -1)) for k in gf])
        prev = np.where(prev[:, 0] == stepno - 1, prev[:, 1], -1)
        Wd = base + ref.BONUS * ((cols[None, :] == prev[:, None]) & (base > 0))
        m = got["match"][gf]
        on = np.flatnonzero(m >= 0)
        assert np.isin(m[on], cols).all() and len(set(m[on].tolist())) == len(on)
        w = Wd[on, np.searchsorted(cols, m[on])]
        assert (w > 0).all()
        r, c = linear_sum_assignment(Wd, maximize=True)
        assert int(w.sum()) == int(Wd[r, c].sum())
        for k, d in zip(np.asarray(gf)[on], m[on]):
            last[frame_gt[k]] = (stepno, int(d))


# ---------------------------------------------------------------------------
# the seeded table: cells of one, two and three ground truths, a cell of many
# detection tracks and one of many ground truths (both beyond a wavefront), empty
# sides; ground-truth tracks of 63, 64 and 65 frames across a tile edge, with holes
# ---------------------------------------------------------------------------
CELLS = [(3, 1), (5, 2), (6, 3), (0, 2), (2, 0), (70, 5), (4, 66)]
LENGTHS = [1, 7, 63, 64, 65, 130]
THR = 0.1


@pytest.fixture(scope="module")
def seeded():
    """(flat, keep, vis, the restatement with keep)."""
    f = hota_ref.seeded_flat(23, CELLS, LENGTHS)
    # the cell of 70 detection tracks: all of them on the positions of its longest
    # ground truth from the first on, with that ground truth's box on every frame --
    # 70 equal candidates on its first frame
    cell = int(np.flatnonzero(np.asarray(f.cell_unit) == 5)[0])      # (cells lie category-major)
    d0, d1 = int(f.cell_dt_off[cell]), int(f.cell_dt_off[cell + 1])
    assert d1 - d0 == 70
    f.dt_frame_box = np.array(f.dt_frame_box, dtype=np.float64).reshape(-1, 4)
    f.gt_frame_box = np.array(f.gt_frame_box, dtype=np.float64).reshape(-1, 4)
    f.dt_frame_pos, f.gt_flags = np.array(f.dt_frame_pos), np.array(f.gt_flags)
    rows = np.arange(f.cell_gt_off[cell], f.cell_gt_off[cell + 1])
    g = int(rows[np.argmax(np.diff(f.gt_frame_off)[rows])])
    gpos = f.gt_frame_pos[f.gt_frame_off[g]:f.gt_frame_off[g + 1]].tolist()
    for d in range(d0, d1):
        s, e = int(f.dt_frame_off[d]), int(f.dt_frame_off[d + 1])
        f.dt_frame_pos[s:e] = (gpos + list(range(gpos[-1] + 1, gpos[-1] + 1 + e - s)))[:e - s]
    f.dt_frame_box[f.dt_frame_off[d0]:f.dt_frame_off[d1]] = [0, 0, 8, 8]
    f.gt_flags[g] = 0
    f.gt_frame_box[f.gt_frame_off[g]:f.gt_frame_off[g + 1]] = [0, 0, 8, 8]
    keep = (np.random.default_rng(3).random(len(f.dt_cat)) < 0.85).astype(np.uint8)
    keep[d0:d1] = 1
    vis = np.random.default_rng(4).choice([0.0, 0.05, 0.1, 0.5, 0.8, 1.0, np.nan],
                                          len(f.gt_frame_pos))
    want = ref.stage(f, THR, keep, vis, association_ref.VIS_RNG)
    for k in STORE + WALKED:
        want[k].setflags(write=False)
    return f, keep, vis, want


def test_candidates_on_the_seeded_table(seeded):
    f, keep, vis, want = seeded
    # the cases are there
    n = np.diff(want["cand_off"])
    assert {0, 1, 2} <= set(n.tolist()) and n.max() >= 65
    assert ((want["step"] == 1) & (n == 0)).any() and not keep.all()
    frame_gt = np.repeat(np.arange(len(f.gt_frame_off) - 1), np.diff(f.gt_frame_off))
    ignored = (np.asarray(f.gt_flags)[frame_gt] & 1) != 0
    assert ignored.any() and not want["step"][ignored].any() and not n[ignored].any()
    assert {63, 64, 65} <= set(np.diff(f.gt_frame_off).tolist())
    gaps = np.diff(f.gt_frame_pos)
    assert (gaps[gaps > 0] > 1).any() and (np.diff(f.dt_frame_pos) > 1).any()
    got = _device_candidates(f, THR, keep)
    _same(got, want, STORE)
    # in ascending row within a frame; without keep, another store
    for k in np.flatnonzero(n > 1)[::7]:
        assert (np.diff(got["cand_row"][got["cand_off"][k]:got["cand_off"][k + 1]]) > 0).all()
    every = _device_candidates(f, THR, None, fill=77, with_iou=False)
    _same(every, ref.candidates(f, THR, None), STORE[:3] + STORE[4:])
    assert len(every["cand_row"]) > len(got["cand_row"]) and (every["cand_iou"] == 77).all()


def test_all_stages_on_the_seeded_table_twice(seeded):
    f, keep, vis, want = seeded
    got = _device_stage(f, THR, keep, vis, association_ref.VIS_RNG)
    _same(got, want, STORE + WALKED)
    _check_steps(f, got, want)
    for k in ("cat_counts", "vis_counts"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    assert want["cat_counts"][:, 0].all() and want["sw"].any()
    # (its ground truths seldom overlap: the steps of several rows and columns are
    # few here and the business of the contested table below)
    assert sum(len(s[2]) > 1 and len(s[3]) > 1 for s in want["steps"]) > 5
    # determinism: the same bytes from a second run over other junk
    again = _device_stage(f, THR, keep, vis, association_ref.VIS_RNG, fill=77)
    for k in STORE + WALKED + ("cat_counts", "vis_counts"):
        assert again[k].tobytes() == got[k].tobytes(), k
    # match_iou and cand_iou may be NULL
    lean = _device_walk(f, got, with_iou=False)
    assert np.array_equal(lean["match"], got["match"]) and (lean["match_iou"] == -3).all()
    assert np.array_equal(lean["sw"], got["sw"])
    # no windows
    cc, vc = _device_reduce(f, got, got["match"], got["sw"], got["gt_clear"])
    assert np.array_equal(cc, want["cat_counts"]) and vc.shape == (0, 3, 4)


def test_all_stages_on_a_contested_table():
    f = ref.crowded_flat(41, [(3, 1), (5, 2), (6, 3), (9, 4), (4, 4), (70, 3), (3, 66), (8, 6)],
                         length=70)
    keep = (np.random.default_rng(5).random(len(f.dt_cat)) < 0.9).astype(np.uint8)
    want = ref.stage(f, 0.3, keep)
    many = [s for s in want["steps"] if len(s[2]) > 1 and len(s[3]) > 1]
    assert len(many) > 300 and sum((s[4] > ref.BONUS).sum() > 1 for s in many) > 100
    assert want["sw"].sum() > 50 and (want["gt_clear"][:, 3] > 1).any()
    got = _device_stage(f, 0.3, keep)
    _same(got, want, STORE + WALKED)
    _check_steps(f, got, want)
    assert np.array_equal(got["cat_counts"], want["cat_counts"])


def test_all_stages_on_boxes_that_are_any_double():
    prng = np.random.default_rng(79)
    turn = [0]

    def boxes(n):
        kind = boxpop.KINDS[turn[0] % len(boxpop.KINDS)]
        turn[0] += 1
        return boxpop.box_population(kind, 2 * n, prng)
    f = hota_ref.seeded_flat(94, CELLS[:6], [1, 7, 20, 65], boxes=boxes)
    with np.errstate(all="ignore"):
        every = orclib.bb_iou(np.asarray(f.dt_frame_box)[:2000], np.asarray(f.gt_frame_box)[:500])
    assert np.isnan(every).any()
    vis = np.resize([0.05, 0.5, np.nan, 1.0], len(f.gt_frame_pos))
    want = ref.stage(f, 0.05, None, vis, association_ref.VIS_RNG)
    assert want["cat_counts"][:, 0].any() and len(want["cand_row"]) > 50
    got = _device_stage(f, 0.05, None, vis, association_ref.VIS_RNG)
    _same(got, want, STORE + WALKED)
    for k in ("cat_counts", "vis_counts"):
        assert np.array_equal(got[k], want[k]), k


# ---------------------------------------------------------------------------
# the walk alone on given candidate tables: no boxes
# ---------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 65), (2, 2), (3, 2), (2, 3), (63, 64), (64, 64), (65, 64), (3, 128),
          (3, 129), (129, 3), (2, 257)]
# (a step's candidates are staged in LDS up to 64 of them: cells whose tracks all
# stay, with 64 and with more candidates a step)
STAGE_EDGE = [(8, 8), (8, 9), (4, 16), (4, 17)]
FAMILIES = ["dense", "sparse", "equal", "rotate", "alternate"]


def _chain_table(scripts, n_cat=3):
    """A table without boxes from scripts = [(D, [ignored g], {(g, p): (step bit,
    [(row, q)])})] per cell."""
    t = SimpleNamespace(n_cells=len(scripts), cat_ids=np.arange(n_cat, dtype=np.int64))
    G = [1 + max(g for g, _ in sc[2]) for sc in scripts]
    t.cell_dt_off = np.r_[0, np.cumsum([sc[0] for sc in scripts])].astype(np.int32)
    t.cell_gt_off = np.r_[0, np.cumsum(G)].astype(np.int32)
    t.gt_cat = np.repeat(np.arange(len(scripts)) % n_cat, G).astype(np.int32)
    flags, foff, pos, step, lists = [], [0], [], [], []
    for (D, ignored, frames), ng in zip(scripts, G):
        for g in range(ng):
            flags.append(int(g in ignored))
            for p in sorted(p for gg, p in frames if gg == g):
                pos.append(p)
                step.append(frames[(g, p)][0])
                lists.append(sorted(frames[(g, p)][1]))
            foff.append(len(pos))
    t.gt_flags = np.array(flags, np.uint8)
    t.gt_frame_off, t.gt_frame_pos = np.array(foff, np.int32), np.array(pos, np.int32)
    flat = [c for ls in lists for c in ls]
    c = dict(cand_off=np.r_[0, np.cumsum([len(ls) for ls in lists])].astype(np.int64),
             cand_row=np.array([x[0] for x in flat], np.int32),
             cand_q=np.array([x[1] for x in flat], np.int32),
             cand_iou=np.array([x[1] / ONE for x in flat], np.float64),
             step=np.array(step, np.uint8))
    return t, c


def _family(name, seed):
    rng = np.random.default_rng(seed)
    scripts = []
    for n, (G, D) in enumerate(SHAPES + STAGE_EDGE):
        n_pos = 4 + n % 3                                    # 3 to 5 steps and one that is none
        ignored = [1] if G >= 3 and n % 2 and n < len(SHAPES) else []
        frames = {}
        for p in range(n_pos):
            bit = int(p != 2)
            for g in range(G):
                if G > 1 and n < len(SHAPES) and rng.random() < 0.25 and not (g == 0 and p == 0):
                    continue                                 # tracks come and go
                if name == "dense":
                    ls = [(d, int(rng.integers(1, ONE + 1))) for d in range(D)]
                elif name == "sparse":
                    ls = [(d, int(rng.integers(1, ONE + 1))) for d in range(D)
                          if rng.random() < max(0.1, 1.5 / D)]
                elif name == "equal":
                    ls = [(d, ONE // 2) for d in range(D)]
                elif name == "rotate":
                    ls = [(d, ONE if d == (g + p) % D else int(rng.integers(1, ONE // 64)))
                          for d in range(D)]
                else:
                    a, b = g % D, (g + 1) % D
                    ls = [(a, ONE if p % 2 else ONE // 3)]
                    if b != a and p != 3:
                        ls.append((b, ONE // 3 if p % 2 else ONE))
                frames[(g, p)] = (bit, ls)
        scripts.append((D, ignored, frames))
    return _chain_table(scripts)


@pytest.mark.parametrize("name", FAMILIES)
def test_walk_on_given_candidate_tables(name):
    t, c = _family(name, 31 + len(name))
    want = ref.walk(t, c)
    # the family holds what it is for: every shape in a chain of steps
    G, D = np.diff(t.cell_gt_off), np.diff(t.cell_dt_off)
    assert list(zip(G.tolist(), D.tolist())) == SHAPES + STAGE_EDGE
    per_cell = np.bincount([s[0] for s in want["steps"]], minlength=len(G))
    assert (per_cell >= (2 if name == "sparse" else 3)).sum() >= len(G) - 2
    if name in ("dense", "equal", "rotate"):
        sizes = {int((s[4] > 0).sum()) for s in want["steps"]}
        assert {64, 68, 72} <= sizes
    if name != "sparse":
        assert any(any(p >= 0 for p in s[5]) and len(s[2]) > 64 for s in want["steps"])
    if name in ("dense", "equal", "rotate"):
        assert max(len(s[3]) for s in want["steps"]) == 257
    if name == "equal":
        assert all(len(set((s[4] % ref.BONUS).ravel().tolist())) == 1 for s in want["steps"])
    if name == "rotate":
        # every bonus is contested: the row of the step before against a full weight
        assert sum(((s[4] > ref.BONUS) & (s[4] < ref.BONUS + ONE // 64)).any()
                   for s in want["steps"]) > 20
    if name == "alternate":
        assert want["sw"].any() and (want["gt_clear"][:, 3] > 1).any()
    got = _device_walk(t, c)
    _check_steps(t, got, want)
    _same(got, want, WALKED)
    assert (got["match"] >= 0).sum() > 300 and (got["gt_clear"][t.gt_flags != 0] == 0).all()
    # a step that is none changes nothing and matches nothing
    assert (got["match"][c["step"] == 0] == -1).all() and (c["step"] == 0).sum() > 100


def test_walk_refuses_a_cell_beyond_the_potentials():
    """The smaller side of the one cell is 2^18 + 1: status 2, nothing walked.  No
    frame has a candidate, so the tables stay small."""
    n = _lib.TRACK_CLEAR_NMAX + 1
    t = SimpleNamespace(n_cells=1, cat_ids=np.arange(1),
                        cell_dt_off=np.array([0, n], np.int32),
                        cell_gt_off=np.array([0, n], np.int32), gt_flags=np.zeros(n, np.uint8),
                        gt_frame_off=np.r_[0, 1, np.ones(n - 1, np.int64)].astype(np.int32),
                        gt_frame_pos=np.zeros(1, np.int32))
    c = dict(cand_off=np.zeros(2, np.int64), cand_row=np.zeros(0, np.int32),
             cand_q=np.zeros(0, np.int32), cand_iou=None, step=np.ones(1, np.uint8))
    got = _device_walk(t, c)
    assert got["status"] == 2 and got["match"].tolist() == [-1] and not got["gt_clear"].any()


# ---------------------------------------------------------------------------
# the chunk edges of the walk of one ground truth
# ---------------------------------------------------------------------------
def _edge_scripts():
    scripts, notes = [], []
    small, big = ONE // 3, ONE // 2
    for L in (63, 64, 65, 128, 129):
        for e in (62, 63, 64, 127, 128):
            if e >= L:
                continue
            # the follower changes exactly at frame e: row 0 before, row 1 alone there,
            # both behind it (the bonus holds row 1 against row 0's greater q)
            fr = {(0, 2 * k): (1, [(0, big)] if k < e else [(1, small)] if k == e
                               else [(0, big), (1, small)]) for k in range(L)}
            scripts.append((3, [], fr))
            notes.append(("change", L, e))
            # frame e is no step (its candidates are junk): row 0's bonus survives it
            fr = {(0, 2 * k): (int(k != e), [(0, small)] if k < e else [(2, ONE)] if k == e
                               else [(0, small), (1, big)]) for k in range(L)}
            scripts.append((3, [], fr))
            notes.append(("hole", L, e))
            # frame e is a step without a candidate: the bonus is lost, row 1 takes over
            fr = {(0, 2 * k): (1, [(0, small)] if k < e else [] if k == e
                               else [(0, small), (1, big)]) for k in range(L)}
            scripts.append((3, [], fr))
            notes.append(("lost", L, e))
    return scripts, notes


def test_walk_of_one_ground_truth_at_the_chunk_edges():
    scripts, notes = _edge_scripts()
    rng = np.random.default_rng(7)
    for L in (63, 64, 65, 128, 129, 200):                   # and random chains of every length
        scripts.append((5, [], {(0, 3 * k): (int(rng.random() < 0.85),
                                             [(d, int(rng.integers(1, 4)) * (ONE // 4))
                                              for d in range(5) if rng.random() < 0.4])
                                for k in range(L)}))
    t, c = _chain_table(scripts)
    want = ref.walk(t, c)
    got = _device_walk(t, c)
    _same(got, want, WALKED)
    for (kind, L, e), g in zip(notes, range(len(notes))):
        m = got["match"][t.gt_frame_off[g]:t.gt_frame_off[g + 1]]
        row = got["gt_clear"][g].tolist()
        if kind == "change":
            assert m.tolist() == [0] * e + [1] * (L - e) and row == [L, L, 1, 1], (kind, L, e)
        elif kind == "hole":
            assert m.tolist() == [0] * e + [-1] + [0] * (L - e - 1), (kind, L, e)
            assert row == [L, L - 1, 0, 1], (kind, L, e)
        else:
            assert m.tolist() == [0] * e + [-1] + [1] * (L - e - 1), (kind, L, e)
            assert row == [L, L - 1, int(e + 1 < L), 1 + int(e + 1 < L)], (kind, L, e)
    assert want["sw"][t.gt_frame_off[len(notes)]:].sum() > 20


# ---------------------------------------------------------------------------
# the reduction alone on synthetic tables
# ---------------------------------------------------------------------------
def test_reduce_on_synthetic_tables():
    rng = np.random.default_rng(17)
    n_cat, G = 3, [2, 1, 4, 3, 70, 5, 6]
    cat = [c % n_cat for c in range(len(G))]
    cat[3], cat[5] = -1, n_cat                               # two cells count nowhere
    L = [int(rng.choice([0, 1, 7, 63, 64, 65, 130])) for _ in range(sum(G))]
    t = SimpleNamespace(n_cells=len(G), cat_ids=np.arange(n_cat, dtype=np.int64))
    t.cell_dt_off = (np.arange(len(G) + 1) * 6).astype(np.int32)
    t.cell_gt_off = np.r_[0, np.cumsum(G)].astype(np.int32)
    t.gt_cat = np.repeat(cat, G).astype(np.int32)
    t.gt_flags = ((rng.random(sum(G)) < 0.25) | 2 * rng.integers(0, 2, sum(G))).astype(np.uint8)
    t.gt_frame_off = np.r_[0, np.cumsum(L)].astype(np.int32)
    n_gf = int(t.gt_frame_off[-1])
    t.gt_frame_pos = np.zeros(n_gf, np.int32)
    lists = [sorted(rng.choice(6, int(rng.integers(0, 5)), replace=False).tolist())
             for _ in range(n_gf)]
    flat = [d for ls in lists for d in ls]
    c = dict(cand_off=np.r_[0, np.cumsum([len(ls) for ls in lists])].astype(np.int64),
             cand_row=np.array(flat, np.int32),
             cand_q=rng.integers(1, ONE + 3, len(flat)).astype(np.int32), cand_iou=None)
    c["cand_q"][::11] = rng.integers(-2, 1, len(c["cand_q"][::11]))      # no candidates
    # a match of the list, one that is not in it, none
    match = np.array([int(rng.choice(ls + [7, -1, -1])) if ls else int(rng.choice([-1, 3]))
                      for ls in lists], np.int32)
    sw = (rng.random(n_gf) < 0.2).astype(np.uint8) * rng.integers(1, 255, n_gf).astype(np.uint8)
    present = np.array(L)
    matched = np.array([int(rng.choice([0, l // 5, (l + 4) // 5, 4 * l // 5, 4 * l // 5 + 1, l]))
                        for l in L])
    gt_clear = np.stack([present, matched, rng.integers(0, 9, len(L)),
                         rng.integers(0, 4, len(L))], 1).astype(np.int32)
    vis = rng.choice([0.0, 0.05, 0.1, 0.5, 0.8, 1.0, np.nan], n_gf)
    windows = association_ref.VIS_RNG + [[0.5, 0.5], [0.05, 0.1], [2, 3]]
    assert len(windows) == 8 and (t.gt_flags & 1).any() and (c["cand_q"] <= 0).any()
    want = ref.reduce(t, c, match, sw, gt_clear, vis, windows, n_cat)
    assert want[0].any(0).all() and want[1][:7].any(1).all() and not want[1][7].any()
    got = _device_reduce(t, c, match, sw, gt_clear, vis, windows, n_cat)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w)
    again = _device_reduce(t, c, match, sw, gt_clear, vis, windows, n_cat, fill=77)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    # mostly tracked / partly / mostly lost at their integer edges
    k = np.flatnonzero(((t.gt_flags & 1) == 0) & (t.gt_cat >= 0) & (t.gt_cat < n_cat))
    mt = 5 * matched[k] > 4 * present[k]
    ml = 5 * matched[k] < present[k]
    assert got[0][:, 3].sum() == mt.sum() and got[0][:, 5].sum() == ml.sum()
    assert got[0][:, 3:6].sum() == len(k)


# ---------------------------------------------------------------------------
# the hand-written table, the empty sides, the refusals
# ---------------------------------------------------------------------------
def test_all_stages_on_the_hand_written_table():
    f, dt_at, gt_at, keep, vis = ref.hand_flat()
    got = _device_stage(f, ref.HAND_THR, keep, vis, ref.HAND_VIS_RNG)
    assert got["status"] == 0
    assert ref.by_given(f, dt_at, gt_at, got["match"], rows=True) == ref.HAND_MATCH
    assert ref.by_given(f, dt_at, gt_at, got["sw"]) == ref.HAND_SW
    assert got["gt_clear"][gt_at].tolist() == ref.HAND_GT_CLEAR
    assert got["cat_counts"].tolist() == [r[4:] for r in ref.HAND_CAT_COUNTS]
    assert got["vis_counts"].tolist() == ref.HAND_VIS_COUNTS
    iou = ref.by_given(f, dt_at, gt_at, got["match_iou"] * 10)
    assert iou[:9] == [6, 6, 10, 10, 0, 10, 6, 0, 6]
    above = _device_stage(f, ref.HAND_THR_ABOVE, keep)
    assert above["cat_counts"].tolist() == [r[4:] for r in ref.HAND_CAT_COUNTS_ABOVE]


@pytest.mark.parametrize("case", ["no_detection_tracks", "no_ground_truth", "no_cells",
                                  "no_detection_frames", "mixed"])
def test_all_stages_on_empty_sides(case):
    f, vis = association_ref.empty_sides()[case]
    want = ref.stage(f, 0.5, None, vis, association_ref.VIS_RNG)
    got = _device_stage(f, 0.5, None, vis, association_ref.VIS_RNG)
    _same(got, want, STORE + WALKED)
    for k in ("cat_counts", "vis_counts"):
        assert np.array_equal(got[k], want[k]), k
    if case != "mixed":
        assert not want["cat_counts"][:, :3].any() and (want["match"] == -1).all()
        assert not want["step"].any()
    else:
        # the long ground truth is followed on the frames the two tracks with boxes have
        assert want["cat_counts"][:, 0].any() and (want["match"] >= 0).sum() > 10


def test_argument_refusals_launch_nothing():
    import torch
    lib = _lib.load()
    f, _, _, keep, vis = ref.hand_flat()
    sizes = _sizes(f)
    n_dt, n_gt, n_cells, _, n_gf = sizes
    hold, ptrs = _cand_tables(f, keep)
    c = ref.candidates(f, 0.5, keep)
    n_cand = len(c["cand_row"])
    off = _junk((n_gf + 1,), torch.int64, 77)
    step = _junk((n_gf,), torch.uint8, 77)
    row, q = _junk((n_cand,), torch.int32, 77), _junk((n_cand,), torch.int32, 77)
    mt, sw = _junk((n_gf,), torch.int32, 77), _junk((n_gf,), torch.uint8, 77)
    gc, status = _junk((n_gt, 4), torch.int32, 77), _junk((1,), torch.int32, 77)
    cc, vc = _junk((2, 7), torch.int64, 77), _junk((9, 2, 4), torch.int64, 77)
    good = _store_ptrs(c, hold)
    gstep = _up(c["step"], np.uint8)
    cols = [_up(f.gt_cat, np.int32), _up(f.gt_flags, np.uint8), _up(f.gt_frame_off, np.int32)]
    visd, rngd = _up(vis, np.float64), _up(np.resize(ref.HAND_VIS_RNG, (9, 2)), np.float64)
    ws = _ws(sizes)

    def count(thr=0.5, nbytes=ws.nbytes):
        return lib.taoamd_track_clear_count(*sizes, thr, *ptrs, off.data_ptr(), step.data_ptr(),
                                            ws.data_ptr(), nbytes, _stream())

    def fill(thr=0.5, nbytes=ws.nbytes):
        return lib.taoamd_track_clear_fill(*sizes, thr, *ptrs, good[0], n_cand, row.data_ptr(),
                                           q.data_ptr(), None, ws.data_ptr(), nbytes, _stream())

    def walk(nbytes=ws.nbytes):
        return lib.taoamd_track_clear_walk(
            n_dt, n_gt, n_cells, n_gf, n_cand, ptrs[0], ptrs[1], ptrs[2], ptrs[7], ptrs[8],
            *good[:3], None, gstep.data_ptr(), mt.data_ptr(), None, sw.data_ptr(), gc.data_ptr(),
            status.data_ptr(), ws.data_ptr(), nbytes, _stream())

    def reduce(n_vis=3, vis_ptr=visd.data_ptr(), nbytes=ws.nbytes):
        return lib.taoamd_track_clear_reduce(
            n_dt, n_gt, n_gf, n_cand, 2, n_vis, *[x.data_ptr() for x in cols], vis_ptr,
            rngd.data_ptr(), *good[:3], mt.data_ptr(), sw.data_ptr(), gc.data_ptr(),
            cc.data_ptr(), vc.data_ptr(), ws.data_ptr(), nbytes, _stream())
    for bad in (0.0, -1.0, 1.0 + 2.0 ** -52, float("nan")):
        assert count(bad) == _lib.ERR_ARG and fill(bad) == _lib.ERR_ARG, bad
    assert reduce(n_vis=9) == _lib.ERR_ARG and reduce(vis_ptr=None) == _lib.ERR_ARG
    short = ws.nbytes - 1
    assert count(nbytes=short) == 4 and fill(nbytes=short) == 4
    assert walk(nbytes=short) == 4 and reduce(nbytes=short) == 4
    ws.check()
    for x in (off, step, row, q, mt, sw, gc, status, cc, vc):
        assert bool((x == 77).all())
    # the good calls succeed
    assert count() == _lib.OK and fill() == _lib.OK and walk() == _lib.OK
    assert reduce() == _lib.OK
    ws.check()
    assert int(status.item()) == 0 and np.array_equal(off.cpu().numpy(), c["cand_off"])
    assert np.array_equal(row.cpu().numpy(), c["cand_row"])
    assert cc.cpu().numpy().tolist() == [r[4:] for r in ref.HAND_CAT_COUNTS]
    assert vc[:3].cpu().numpy().tolist() == ref.HAND_VIS_COUNTS and bool((vc[3:] == 77).all())


# ---------------------------------------------------------------------------
# the class API
# ---------------------------------------------------------------------------
def _tao(name, **kw):
    from tao_amodal_amd import flatten
    from tao_amodal_amd.columns import DTColumns
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval, TaoResults
    dt = DTColumns.from_json(path(name, "pred.json"))
    dt.track_id, _ = flatten.make_track_ids_unique(dt)
    gt = Tao(path(name, "gt.json"))
    return TaoEval(gt, TaoResults(gt, dt), **kw)


@pytest.mark.parametrize("name", ["f1", "f4"])
def test_class_api_on_the_fixtures(name):
    from tao_amodal_amd.evaluation.tao_amodal import followers
    ev = _tao(name)
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.clear()
    ev.evaluate()
    ev.accumulate()
    before = {k: ev.eval[k].copy() for k in ("precision", "recall")}
    flat = ev._run.flat
    ident = identity_ref.identity(flat, 0.5)
    keep = ident["kept"].astype(np.uint8)
    vis = np.asarray(ev._gt_columns.ann_vis, dtype=np.float64)[flat.gt_frame_box.index]
    windows = association_ref.VIS_RNG
    want = ref.stage(flat, 0.5, keep, vis, windows)
    cats = np.asarray(flat.cat_ids).tolist()
    pos = [cats.index(int(c)) for c in ev.params.cat_ids]
    got = ev.clear()
    K = len(ev.params.cat_ids)
    assert "frames" not in got and "tracks" not in got and got["frame_thr"] == 0.5
    assert got["vis_rng"] == windows and len(got["vis_lbl"]) == 5
    cc = np.concatenate([ident["cat_counts"][pos][:, :4], want["cat_counts"][pos]], 1)
    assert got["cat_counts"].dtype == np.int64 and np.array_equal(got["cat_counts"], cc)
    assert got["cat_counts"].shape == (K, 11) and cc[:, 4].any()
    assert np.array_equal(got["cat_counts"][:, :4], ev.identity()["cat_counts"][:, :4])
    assert np.array_equal(got["fn"], cc[:, 1] - cc[:, 4]) and (got["fn"] >= 0).all()
    assert np.array_equal(got["fp"], cc[:, 3] - cc[:, 4]) and (got["fp"] >= 0).all()
    assert np.array_equal(cc[:, 7:10].sum(1), cc[:, 0])
    r = followers.clear_ratios(cc)
    rr = ref.ratios(cc)
    has = (cc[:, 1] + cc[:, 3]) > 0
    for k in ref.RATIOS:
        w = np.where(has, r[k], np.nan)
        assert got[k].dtype == np.float64 and got[k].tobytes() == w.tobytes(), k
        assert np.array_equal(r[k], rr[k]), k
        assert got["mean"][k] == float(r[k][has].mean()), k
    assert np.array_equal(got["vis_counts"], want["vis_counts"][:, pos])
    assert got["vis_counts"].shape == (5, K, 4)
    assoc = ev.association(frame_thr=0.5)
    assert np.array_equal(got["vis_counts"][..., 0], assoc["vis_counts"][..., 0])
    assert (got["cat_counts"][:, 4] <= assoc["cat_counts"][:, 2]).all()
    with np.errstate(all="ignore"):
        re_ = np.where(got["vis_counts"][..., 0] > 0,
                       got["vis_counts"][..., 1] / got["vis_counts"][..., 0], np.nan)
    assert np.array_equal(got["vis_re"], re_, equal_nan=True)
    tot = got["total"]
    rt = followers.clear_ratios(cc.sum(0))
    assert tot["tp"] == cc[:, 4].sum() and tot["fn"] == got["fn"].sum()
    assert all(tot[k] == float(rt[k]) for k in ref.RATIOS) and tot["mota"] <= 1
    assert np.array_equal(tot["vis_counts"], got["vis_counts"].sum(1))
    assert ev.clear()["fn"] is got["fn"]                                       # cached
    full = ev.clear(per_track=True, per_frame=True)
    assert full["fn"] is got["fn"]
    gid, tr = full["tracks"]
    gc = want["gt_clear"].astype(np.int64)
    assert np.array_equal(gid, np.asarray(flat.gt_id))
    assert np.array_equal(tr[:, :3], gc[:, :3])
    assert np.array_equal(tr[:, 3], np.maximum(gc[:, 3] - 1, 0))
    live = (np.asarray(flat.gt_flags) & 1) == 0
    mt = 5 * gc[:, 1] > 4 * gc[:, 0]
    pt = ~mt & (5 * gc[:, 1] >= gc[:, 0])
    assert np.array_equal(tr[:, 4], np.where(live, 2 * mt + pt, 0))
    gid, img, did, s, sw = full["frames"]
    foff, cell, want_img = followers._gt_frame_tables(flat)
    g_of = np.repeat(np.arange(len(foff) - 1), np.diff(foff))
    assert np.array_equal(gid, np.asarray(flat.gt_id)[g_of]) and np.array_equal(img, want_img)
    assert np.array_equal(did, followers._follower_ids(flat, cell, want["match"]))
    assert np.array_equal(s, want["match_iou"]) and (did >= 0).sum() == (s > 0).sum() > 0
    assert np.array_equal(sw, want["sw"]) and sw.dtype == np.uint8
    lines = ev.clear_lines()
    assert len(lines) == 4 + 5 and lines[1].split()[:3] == ["MOTA", "MOTP", "MODA"]
    assert lines[1].split() == list(followers.CLEAR_SCALARS + followers.CLEAR_INTEGERS)
    assert lines[2].split()[0] == "total" and lines[3].split()[:2] == ["class", "mean"]
    assert lines[2].split()[-8] == str(int(tot["tp"]))
    # another threshold and other windows: other tables under other keys
    one = ev.clear(frame_thr=0.75, vis_rng=[[0, 0.5]])
    k2 = identity_ref.identity(flat, 0.75)["kept"].astype(np.uint8)
    w2 = ref.stage(flat, 0.75, k2, vis, [[0, 0.5]])
    assert np.array_equal(one["cat_counts"][:, 4:], w2["cat_counts"][pos])
    assert np.array_equal(one["vis_counts"], w2["vis_counts"][:, pos]) and len(ev._clear) == 2
    assert one["vis_lbl"] == ["[0, 0.5]"]
    # the identity was computed on the way and is what identity() returns
    assert np.array_equal(ev.identity()["cat_counts"], ident["cat_counts"][pos])
    # hota() over the same tracks and frame counts
    assert np.array_equal(ev.hota()["cat_counts"], got["cat_counts"][:, :4])
    for k, v in before.items():
        assert np.array_equal(ev.eval[k], v, equal_nan=True), k


def test_class_api_refusals():
    ev = _tao("f1")
    ev.evaluate()
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="frame_thr"):
            ev.clear(frame_thr=bad)
    with pytest.raises(ValueError, match="vis_rng"):
        ev.clear(vis_rng=[[0, 1]] * 9)
    from tao_amodal_amd import engine
    with pytest.raises(_lib.TaoAmdError, match="visibility windows"):
        engine.stage_track_clear(ev._run.dp, ev._run.ws, 0.5, [[0, 1]] * 9)
    pooled = _tao("f1")
    pooled.params.use_cats = 0
    pooled.evaluate()
    with pytest.raises(NotImplementedError, match="use_cats = 0"):
        pooled.clear()
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval
    segm = TaoEval(Tao(path("f6", "gt.json")), path("f6", "pred_rle.json"), iou_type="segm")
    segm.evaluate()
    with pytest.raises(NotImplementedError, match="iou_type='segm'"):
        segm.clear()
    with pytest.raises(_lib.TaoAmdError, match="on boxes"):
        engine.stage_track_clear(segm._run.dp, segm._run.ws, 0.5, None)
    from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
    assert not hasattr(LVISEval, "clear")                   # the track level's alone
    image = ev._run
    kind = image.flat.kind
    image.flat.kind = "lvis"
    with pytest.raises(NotImplementedError, match="track level"):
        ev.clear()
    image.flat.kind = kind
    # a multi-GPU run: its evaluator refuses, and nothing is cached
    from tao_amodal_amd.evaluation._dist import DistRun
    ev._run = DistRun.__new__(DistRun)
    with pytest.raises(NotImplementedError, match=r"clear\(\) in a multi-GPU run"):
        ev.clear()
    with pytest.raises(NotImplementedError, match=r"clear\(\) in a multi-GPU run"):
        ev.clear_lines()
    assert ev._clear == {}
