"""-m gpu: the track-level occlusion episodes (taoamd_track_occlusion_count,
taoamd_track_occlusion_fill, engine.stage_track_occlusion, TaoEval.occlusions)
against the numpy restatement of tests/occlusion_ref.py.  best[] and vis[] go
straight into the two entry points, so any pattern can be stated; everything is
an integer: every comparison is exact."""
import numpy as np
import pytest

import occlusion_ref as ref
import wsguard
from goldenio import path
from tao_amodal_amd import _lib
from test_gpu_association import _tao

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = -3
EDGES4 = (1, 3, 6, 11)
EDGES8 = (1, 2, 3, 5, 6, 10, 11, 71)


def _up(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], dtype=dtype)
    return torch.from_numpy(a).to(DEV)


def _device(tables, n_cat, window, recover, edges, cap=None, status=False, ws_bytes=None):
    """The two entry points on packed tables; the workspace is exactly the size
    reported, behind a guard band; the outputs hold FILL beforehand.  `cap`: the
    records the fill call may store (default: all); the array is longer."""
    import torch
    lib = _lib.load()
    off, vis, best, gt_cat, gt_flags = tables
    n_gt, n_gf = len(off) - 1, len(best)
    e = np.ascontiguousarray(edges, dtype=np.int32)
    cols = [_up(gt_cat, np.int32), _up(gt_flags, np.uint8), _up(off, np.int32),
            _up(vis, np.float64), _up(best, np.int32)]
    gt_occ = torch.full((max(n_gt, 1), 4), FILL, dtype=torch.int32, device=DEV)
    ep_off = torch.full((n_gt + 1,), FILL, dtype=torch.int64, device=DEV)
    counts = torch.full((n_cat, len(e), 11), FILL, dtype=torch.int64, device=DEV)
    need = lib.taoamd_track_occlusion_workspace(n_gt, n_gf, len(e))
    ws = wsguard.Guarded(need if ws_bytes is None else ws_bytes, DEV)
    stream = torch.cuda.current_stream().cuda_stream
    head = (n_gt, n_gf, n_cat, len(e), recover, window[0], window[1], e.ctypes.data,
            *[c.data_ptr() for c in cols])
    st = lib.taoamd_track_occlusion_count(*head, gt_occ.data_ptr(), ep_off.data_ptr(),
                                          counts.data_ptr(), ws.data_ptr(), ws.nbytes, stream)
    if status:
        torch.cuda.synchronize()
        return st
    _lib.check(st, "taoamd_track_occlusion_count")
    n_ep = int(ep_off[-1].item())
    cap = n_ep if cap is None else cap
    episodes = torch.full((max(cap, n_ep) + 8, 9), FILL, dtype=torch.int32, device=DEV)
    _lib.check(lib.taoamd_track_occlusion_fill(
        *head, ep_off.data_ptr(), cap, episodes.data_ptr(), ws.data_ptr(), ws.nbytes, stream),
        "taoamd_track_occlusion_fill")
    ws.check()
    return dict(episodes=episodes.cpu().numpy(), n_ep=n_ep, gt_occ=gt_occ[:n_gt].cpu().numpy(),
                counts=counts.cpu().numpy(), ep_off=ep_off.cpu().numpy())


def _want(tables, n_cat, window, recover, edges):
    off, vis, best, gt_cat, gt_flags = tables
    return ref.occlusions(off, vis, best, gt_cat, gt_flags, n_cat, window[0], window[1], recover,
                          edges)


def _same(got, want):
    n = len(want["episodes"])
    assert got["n_ep"] == n
    for k in ("gt_occ", "counts", "ep_off"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["episodes"][:n], want["episodes"])
    assert (got["episodes"][n:] == FILL).all()


def test_abi_on_the_hand_written_table():
    t, want = ref.hand()
    got = _device(t, 2, ref.HAND_WINDOW, 2, ref.HAND_EDGES)
    assert [tuple(r) for r in got["episodes"][:got["n_ep"]].tolist()] == ref.HAND_EPISODES
    assert got["gt_occ"].tolist() == ref.HAND_GT_OCC
    assert got["ep_off"].tolist() == ref.HAND_EP_OFF
    assert got["counts"].tolist() == ref.HAND_COUNTS
    _same(got, want)
    from tao_amodal_amd.evaluation.tao_amodal import followers
    e = {"columns": {"counts": list(_lib.OCC_COUNT_COLUMNS)}, "counts": got["counts"],
         "len_lbl": ["1", "2", "3+"], "frame_thr": 0.5, "vis_rng": [0.0, 0.1], "recover": 2}
    assert followers.occlusion_lines(e) == ref.HAND_LINES
    one = _device(t, 2, ref.HAND_WINDOW, 1, ref.HAND_EDGES)
    assert tuple(one["episodes"][2].tolist()) == ref.HAND_EPISODE2_RECOVER1
    assert one["counts"][0, 0].tolist() == ref.HAND_COUNTS00_RECOVER1
    _same(one, ref.hand(recover=1)[1])
    # a visibility exactly at lo and exactly at hi
    t, want = ref.hand(tracks=[ref.EDGE_TRACK], window=ref.EDGE_WINDOW)
    got = _device(t, 2, ref.EDGE_WINDOW, 2, ref.HAND_EDGES)
    assert [tuple(r) for r in got["episodes"][:2].tolist()] == ref.EDGE_EPISODES
    _same(got, want)


# ---------------------------------------------------------------------------
# placed episodes: every edge of the chunks of 64 frames a wavefront walks
# ---------------------------------------------------------------------------
def _track(L, runs, best=(), default=5):
    """L frames, occluded (0.05) on the runs (a, n), visible elsewhere; the
    follower `default` but for the (start, stop, value) of `best`."""
    vis, b = np.ones(L), np.full(L, default, np.int32)
    for a, n in runs:
        vis[a:a + n] = 0.05
    for lo, hi, v in best:
        b[lo:hi] = v
    return b.tolist(), vis.tolist()


def _placed():
    alt = _track(129, [(k, 1) for k in range(0, 64, 2)] + [(70, 10), (90, 11), (110, 12)])
    alt = ((np.arange(129) // 3 % 3 - 1).tolist(), alt[1])     # followers -1, 0, 1 in threes
    return [
        # 60 .. 130 across two chunk edges, held counted across them; a recover window
        # that crosses the edge at 192; one cut off by the track's end
        _track(257, [(60, 71), (180, 11), (250, 5)],
               [(70, 100, -1), (100, 110, 6), (125, 129, -1), (191, 196, -1), (255, 257, -1)]),
        # 1010...: 32 episodes in a chunk; lengths 10, 11, 12
        alt,
        # starts at frame 64: entry is frame 63's, through the carry
        _track(127, [(64, 7)], [(0, 63, 6), (63, 68, 7), (68, 127, 8)]),
        # spans frames 63 - 64
        _track(128, [(63, 2)], [(0, 128, 9), (64, 65, -1)]),
        # ends at frame 63, after at frame 64
        _track(65, [(60, 4)], [(0, 65, 7), (60, 64, -1)]),
        # lengths 1, 2, 3, 5, 6 and one that ends the track at frame 63
        _track(64, [(10, 1), (12, 2), (20, 3), (30, 5), (40, 6), (63, 1)]),
        _track(63, [(60, 3)]),
        _track(2, [(1, 1)], [(1, 2, -1)]),
        _track(1, [(0, 1)], default=3),
        _track(0, []),
    ]


PLACED_ROWS = {          # recover: rows (place in _placed(), a, n, outcome, entry, after, gap, covered, held)
    64: [(0, 60, 71, ref.KEPT, 5, 5, 0, 37, 27), (0, 180, 11, ref.KEPT, 5, 5, 5, 11, 11),
         (0, 250, 5, ref.LOST, 5, -1, 0, 5, 5)],
    3: [(0, 180, 11, ref.LOST, 5, -1, 0, 11, 11), (2, 64, 7, ref.SWITCHED, 7, 8, 0, 7, 4),
        (3, 63, 2, ref.KEPT, 9, 9, 0, 1, 1), (4, 60, 4, ref.KEPT, 7, 7, 0, 0, 0),
        (5, 63, 1, ref.END, 5, -1, 0, 1, 1), (8, 0, 1, ref.START, -1, -1, 0, 1, 0)],
    1: [(0, 180, 11, ref.LOST, 5, -1, 0, 11, 11), (4, 60, 4, ref.KEPT, 7, 7, 0, 0, 0)],
}
N_CAT = 3


def _population(n_gt):
    placed = _placed()
    return ref.pack([(i % N_CAT, int(i % 5 == 4)) + placed[i % len(placed)] for i in range(n_gt)])


@pytest.fixture(scope="module")
def placed_want():
    """{(n_gt, recover): (tables, edges, restatement)}, computed once."""
    out = {}
    for n_gt in (0, 1, 3, 4, 5, 257):
        t = _population(n_gt)
        for recover, edges in ((1, (1,)), (3, EDGES4), (64, EDGES8)):
            w = _want(t, N_CAT, (0.0, 0.1), recover, edges)
            for v in w.values():
                v.setflags(write=False)
            out[n_gt, recover] = (t, edges, w)
    return out


@pytest.mark.parametrize("recover", [1, 3, 64])
@pytest.mark.parametrize("n_gt", [0, 1, 3, 4, 5, 257])
def test_abi_on_placed_episodes(placed_want, n_gt, recover):
    t, edges, want = placed_want[n_gt, recover]
    if n_gt == 257:
        # the cases are there: the track lengths, the placed rows, a length on every edge
        assert set(np.diff(t[0]).tolist()) == {0, 1, 2, 63, 64, 65, 127, 128, 129, 257}
        rows = set(tuple(r) for r in want["episodes"][:want["ep_off"][10]].tolist())
        assert all(r in rows for r in PLACED_ROWS[recover])
        assert want["gt_occ"][1, 0] == 32 + 3
        assert set(edges) <= set(want["episodes"][:, 2].tolist())
        assert (want["counts"][:, :, 0].sum(0) > 0).all()
        assert (t[4] & 1).any() and want["gt_occ"][t[4] == 1, 0].sum() > 0
    _same(_device(t, N_CAT, (0.0, 0.1), recover, edges), want)


# ---------------------------------------------------------------------------
# seeded random tracks: Markov runs for occ and for best
# ---------------------------------------------------------------------------
def _random_tracks(seed, n):
    rng = np.random.default_rng(seed)
    hidden = [0.0, 0.05, 0.1]
    shown = [float(np.nextafter(0.1, 1)), 0.5, 1.0, float("nan")]
    out = []
    for i in range(n):
        L = int(rng.choice([0, 1, 2, 17, 63, 64, 65, 127, 128, 129, 200, 257]))
        flip, move = rng.choice([0.03, 0.2, 0.5]), rng.choice([0.02, 0.2, 0.6])
        o, b = bool(rng.random() < 0.5), int(rng.integers(-1, 100))
        best, vis = [], []
        for _ in range(L):
            if rng.random() < flip:
                o = not o
            if rng.random() < move:
                b = int(rng.integers(0, 100)) if rng.random() < 0.7 else -1
            best.append(b)
            vis.append(float(rng.choice(hidden if o else shown)))
        out.append((int(rng.integers(0, 4)), int(rng.random() < 0.2), best, vis))
    return out


@pytest.fixture(scope="module")
def seeded():
    """(tables, {recover: restatement}), computed once."""
    t = ref.pack(_random_tracks(41, 300))
    want = {r: _want(t, 4, (0.0, 0.1), r, EDGES4) for r in (2, 64)}
    for w in want.values():
        for v in w.values():
            v.setflags(write=False)
    return t, want


@pytest.mark.parametrize("recover", [2, 64])
def test_abi_on_seeded_random_tracks(seeded, recover):
    t, want = seeded
    w = want[recover]
    assert len(np.unique(t[2])) > 64 + 1 and np.isnan(t[1]).any()
    assert (np.bincount(w["episodes"][:, 3], minlength=6) > 0).all()
    assert w["episodes"][:, 2].max() > 64 and (w["episodes"][:, 6] > 0).any()
    assert (w["counts"][..., 0].sum(1) > 0).all()
    _same(_device(t, 4, (0.0, 0.1), recover, EDGES4), w)


def test_abi_fill_stores_whole_tracks_below_cap(seeded):
    t, want = seeded
    w = want[2]
    n = len(w["episodes"])
    g = 100 + int(np.argmax(np.diff(w["ep_off"])[100:] >= 2))
    mid = int(w["ep_off"][g]) + 1                           # inside a track's records
    assert 0 < w["ep_off"][g] < mid < w["ep_off"][g + 1]
    for cap in (0, 1, mid, n - 1, n, n + 5):
        got = _device(t, 4, (0.0, 0.1), 2, EDGES4, cap=cap)
        # the tracks with ep_off[g + 1] <= cap, nothing else, nothing at or beyond cap
        stored = int(w["ep_off"][w["ep_off"] <= cap].max())
        assert np.array_equal(got["episodes"][:stored], w["episodes"][:stored]), cap
        assert (got["episodes"][stored:] == FILL).all(), cap
        assert np.array_equal(got["counts"], w["counts"])


def test_abi_error_paths():
    t, _ = ref.hand()
    lib = _lib.load()
    need = lib.taoamd_track_occlusion_workspace(len(t[0]) - 1, len(t[2]), 3)

    def call(window=ref.HAND_WINDOW, recover=2, edges=ref.HAND_EDGES, **kw):
        return _device(t, 2, window, recover, edges, status=True, **kw)
    assert call(recover=0) == 2 and call(recover=65) == 2
    assert call(edges=(2, 3)) == 2 and call(edges=(1, 3, 3)) == 2
    assert call(edges=tuple(range(1, 10))) == 2
    assert call(window=(0.2, 0.1)) == 2 and call(window=(float("nan"), 0.1)) == 2
    assert call(ws_bytes=need - 1) == 4
    assert call() == 0 and call(recover=64, edges=tuple(range(1, 9))) == 0


# ---------------------------------------------------------------------------
# the class API
# ---------------------------------------------------------------------------
def _restated(ev, thr, window, recover, edges):
    """The restatement on association(per_frame=True)'s followers (detection
    track ids: equal ids, equal followers), the category axis in the caller's
    order."""
    a = ev.association(thr, vis_rng=[list(window)], per_frame=True)
    flat = ev._run.flat
    foff, img, best_id, _ = a["frames"]
    vis = np.asarray(ev._gt_columns.ann_vis, dtype=np.float64)[flat.gt_frame_box.index]
    w = ref.occlusions(foff, vis, best_id, np.asarray(flat.gt_cat), np.asarray(flat.gt_flags),
                       len(flat.cat_ids), window[0], window[1], recover, edges)
    cats = np.asarray(flat.cat_ids).tolist()
    pos = [cats.index(int(c)) for c in ev.params.cat_ids]
    ep = w["episodes"].astype(np.int64)
    first = foff[ep[:, 0]] + ep[:, 1]
    return dict(counts=w["counts"][pos], gt_occ=w["gt_occ"].astype(np.int64), episodes=ep,
                first_img=np.asarray(img)[first], last_img=np.asarray(img)[first + ep[:, 2] - 1],
                gt_id=np.asarray(flat.gt_id), vis_counts=a["vis_counts"])


def _check_class_api(ev, window=(0.0, 0.1), recover=3, edges=EDGES4):
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.occlusions()
    ev.evaluate()
    ev.accumulate()
    before = {k: ev.eval[k].copy() for k in ("precision", "recall")}
    got = ev.occlusions(0.5, window, recover, edges)
    want = _restated(ev, 0.5, window, recover, edges)
    K = len(ev.params.cat_ids)
    assert "tracks" not in got and "episodes" not in got
    assert got["columns"] == {"counts": list(ref.COUNT_COLUMNS), "tracks": list(ref.TRACK_COLUMNS),
                              "episodes": list(ref.EPISODE_COLUMNS), "outcomes": list(ref.OUTCOMES)}
    assert got["len_edges"] == list(edges) and got["recover"] == recover
    assert got["vis_rng"] == [float(window[0]), float(window[1])] and got["frame_thr"] == 0.5
    assert got["counts"].shape == (K, len(edges), 11) and got["counts"].dtype == np.int64
    assert np.array_equal(got["counts"], want["counts"])
    # per category, frames and covered over the buckets are the association's window
    assert np.array_equal(got["counts"][:, :, 1:3].sum(1), want["vis_counts"][0, :, :2])
    assert ev.occlusions(0.5, window, recover, edges)["counts"] is got["counts"]       # cached
    full = ev.occlusions(0.5, window, recover, edges, per_track=True, per_episode=True)
    assert full["counts"] is got["counts"]
    ids, tracks = full["tracks"]
    assert np.array_equal(ids, want["gt_id"]) and np.array_equal(tracks, want["gt_occ"])
    gt_id, first, last, ep = full["episodes"]
    assert ep.dtype == np.int64 and np.array_equal(ep, want["episodes"])
    assert np.array_equal(gt_id, want["gt_id"][ep[:, 0]])
    assert np.array_equal(first, want["first_img"]) and np.array_equal(last, want["last_img"])
    lines = ev.occlusion_lines(0.5, window, recover, edges)
    assert len(lines) == 2 + len(edges) and all(isinstance(x, str) for x in lines)
    assert [int(x.split()[1]) for x in lines[2:]] == got["counts"][:, :, 0].sum(0).tolist()
    for k, v in before.items():
        assert np.array_equal(ev.eval[k], v, equal_nan=True), k
    return got, want


def test_class_api_on_the_fixture():
    ev = _tao("f1")
    got, want = _check_class_api(ev)
    assert got["len_lbl"] == ["1-2", "3-5", "6-10", "11+"]
    # every outcome occurs, followers are ids of detection tracks
    assert (got["counts"].sum((0, 1))[4:10] > 0).all()
    ep = want["episodes"]
    assert set(ep[:, 4].tolist()) - {-1} <= set(np.asarray(ev._run.flat.dt_id).tolist())
    # other arguments: another table under another key
    other = ev.occlusions(1.0, (0.1, 0.8), 1, (1, 2))
    assert other["len_lbl"] == ["1", "2+"]
    assert np.array_equal(other["counts"], _restated(ev, 1.0, (0.1, 0.8), 1, (1, 2))["counts"])
    assert ev.occlusions()["counts"] is got["counts"]
    ev.evaluate()                                           # clears the cache
    assert ev.occlusions()["counts"] is not got["counts"]
    assert np.array_equal(ev.occlusions()["counts"], got["counts"])


def test_class_api_on_a_params_subset():
    whole = _tao("f1")
    whole.evaluate()
    all_cats = list(whole.params.cat_ids)
    base = whole.occlusions()
    ev = _tao("f1")
    ev.params.cat_ids = [ev.params.cat_ids[i] for i in (4, 0, 2)]
    got, _ = _check_class_api(ev)
    at = [all_cats.index(c) for c in ev.params.cat_ids]
    assert got["counts"].shape[0] == 3 and np.array_equal(got["counts"], base["counts"][at])


def test_stage_reuses_the_followers_of_its_threshold(monkeypatch):
    from tao_amodal_amd import engine
    ev = _tao("f1")
    ev.evaluate()
    ran = []
    stage = engine.stage_track_association
    monkeypatch.setattr(engine, "stage_track_association",
                        lambda dp, ws, thr, rng: (ran.append((thr, len(rng))), stage(dp, ws, thr, rng))[1])
    one = ev.occlusions(0.5)
    assert ran == [(0.5, 0)]                                # not there yet: run without windows
    ev.occlusions(0.5, recover=1)
    assert ran == [(0.5, 0)]                                # reused
    ev.occlusions(0.75)
    assert ran == [(0.5, 0), (0.75, 0)]
    ev.association(0.5)
    assert len(ran) == 3
    dp, ws = ev._run.dp, ev._run.ws
    engine.stage_track_occlusion(dp, ws, 0.5, 0.0, 0.1, 3, EDGES4)
    assert len(ran) == 3 and ws.occ_n is None
    assert np.array_equal(ws.occ_counts.cpu().numpy()[ev._cat_pos] if ev._cat_pos is not None
                          else ws.occ_counts.cpu().numpy(), one["counts"])


def test_class_api_refusals():
    ev = _tao("f1")
    ev.evaluate()
    for bad in (0.0, 1 + 2.0 ** -52, float("nan")):
        with pytest.raises(ValueError, match="frame_thr"):
            ev.occlusions(bad)
    for bad in ((0.2, 0.1), (float("nan"), 0.1), (0.0, 0.1, 0.2)):
        with pytest.raises(ValueError, match="vis_rng"):
            ev.occlusions(vis_rng=bad)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="recover"):
            ev.occlusions(recover=bad)
    for bad in ((), (2, 3), (1, 3, 3), tuple(range(1, 10)), (1, 2.5)):
        with pytest.raises(ValueError, match="len_edges"):
            ev.occlusions(len_edges=bad)
    from tao_amodal_amd import engine
    with pytest.raises(_lib.TaoAmdError, match="need the frames' visibility"):
        engine.stage_track_occlusion(ev._run.dp, ev._run.ws, 0.5, 0.0, 0.1, 3, EDGES4)
    ev.occlusions()                                         # uploads the visibilities
    with pytest.raises(_lib.TaoAmdError, match="bad argument"):
        engine.stage_track_occlusion(ev._run.dp, ev._run.ws, 0.5, 0.0, 0.1, 65, EDGES4)
    with pytest.raises(_lib.TaoAmdError, match="length buckets"):
        engine.stage_track_occlusion(ev._run.dp, ev._run.ws, 0.5, 0.0, 0.1, 3, range(1, 10))
    pooled = _tao("f1")
    pooled.params.use_cats = 0
    pooled.evaluate()
    with pytest.raises(NotImplementedError, match="use_cats = 0"):
        pooled.occlusions()
    from tao_amodal_amd.evaluation.tao_amodal import Tao, TaoEval
    segm = TaoEval(Tao(path("f6", "gt.json")), path("f6", "pred_rle.json"), iou_type="segm")
    segm.evaluate()
    with pytest.raises(NotImplementedError, match="iou_type='segm'"):
        segm.occlusions()
    with pytest.raises(_lib.TaoAmdError, match="on boxes"):
        engine.stage_track_occlusion(segm._run.dp, segm._run.ws, 0.5, 0.0, 0.1, 3, EDGES4)
