"""The track-level occlusion episodes without a GPU: the numpy restatement
(tests/occlusion_ref.py) on the hand-written table with literal expectations,
and the C ABI's new symbols and refusals (argument and workspace checks come
before the first device call)."""
import os
import re

import numpy as np

import occlusion_ref as ref
from tao_amodal_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_reproduces_the_worked_example():
    best, vis = ref.HAND_TRACKS[0][2], ref.HAND_TRACKS[0][3]
    K, S, L = ref.KEPT, ref.SWITCHED, ref.LOST
    assert (K, S, L) == (3, 4, 5)
    first = [(1, 2, K, 0, 0, 0, 1, 1), (4, 2, S, 0, 1, 0, 2, 1)]
    assert ref.track_episodes(best, vis, 0.0, 0.1, 1) == first + [(7, 1, L, 1, -1, 0, 0, 0)]
    for recover in (2, 3, 64):
        assert ref.track_episodes(best, vis, 0.0, 0.1, recover) \
            == first + [(7, 1, S, 1, 0, 1, 0, 0)]


def test_restatement_reproduces_the_literals():
    t, got = ref.hand()
    assert [tuple(r) for r in got["episodes"].tolist()] == ref.HAND_EPISODES
    assert got["gt_occ"].tolist() == ref.HAND_GT_OCC
    assert got["ep_off"].tolist() == ref.HAND_EP_OFF
    assert got["counts"].tolist() == ref.HAND_COUNTS
    assert got["episodes"].dtype == np.int32 and got["counts"].dtype == np.int64
    # occluded throughout is START although it also ends the track; END needs a follower
    assert ref.HAND_EPISODES[3][3] == ref.START and ref.HAND_EPISODES[4][3] == ref.END
    # the ignored track is in the records and in gt_occ; without it the counts are the same
    assert ref.HAND_TRACKS[4][1] == ref.GT_IGNORE and ref.HAND_GT_OCC[4][0] == 1
    rest = [x for i, x in enumerate(ref.HAND_TRACKS) if i != 4]
    assert np.array_equal(ref.hand(tracks=rest)[1]["counts"], got["counts"])
    # recover = 1: one record, one row of gt_occ's sums and one count row differ
    _, one = ref.hand(recover=1)
    want = list(ref.HAND_EPISODES)
    want[2] = ref.HAND_EPISODE2_RECOVER1
    assert [tuple(r) for r in one["episodes"].tolist()] == want
    assert one["gt_occ"][0].tolist() == ref.HAND_GT_OCC0_RECOVER1
    assert one["counts"][0, 0].tolist() == ref.HAND_COUNTS00_RECOVER1
    assert np.array_equal(one["counts"][1], got["counts"][1])
    # the sums the tables share
    c = got["counts"]
    assert c[..., 0].sum() == len(ref.HAND_EPISODES) - 1
    assert np.array_equal(c[..., 4:10].sum(-1), c[..., 0])
    assert (c[..., 3] <= c[..., 2]).all() and (c[..., 2] <= c[..., 1]).all()


def test_restatement_at_the_window_edges_and_on_a_nan():
    _, got = ref.hand(tracks=[ref.EDGE_TRACK], window=ref.EDGE_WINDOW)
    assert [tuple(r) for r in got["episodes"].tolist()] == ref.EDGE_EPISODES
    # the NaN of track 3 splits its run in two
    assert [e[1:3] for e in ref.HAND_EPISODES if e[0] == 3] == [(1, 1), (3, 1)]
    # the last bucket is open; a length on an edge belongs to the bucket it opens
    for n, j in ((1, 0), (2, 1), (3, 2), (9, 2)):
        _, g = ref.hand(tracks=[(0, 0, [0] * (n + 2), [1] + [0] * n + [1])])
        assert g["counts"][0, :, 0].tolist() == [int(i == j) for i in range(3)]


def _stubbed(cat_ids=(10, 20), cat_pos=None):
    """A TaoEval over a pass that answers the hand-written table: a cell per
    ground-truth track in one video, its detection tracks the rows 10 g .. 10 g +
    9 with the ids 1000 + row, the image of timeline position p is 500 + p."""
    import types
    from tao_amodal_amd.evaluation.tao_amodal import TaoEval
    t, table = ref.hand(recover=2)
    n_gt = len(t[0]) - 1
    calls = []

    def occlusion_table(frame_thr, vis_rng, recover, len_edges, ann_vis):
        calls.append((frame_thr, tuple(vis_rng), recover, tuple(len_edges)))
        return {k: table[k] for k in ("gt_occ", "counts", "episodes")}
    flat = types.SimpleNamespace(
        gt_id=np.arange(n_gt) + 70, dt_id=np.arange(10 * n_gt) + 1000, gt_frame_off=t[0],
        gt_cell=np.arange(n_gt), cell_unit=np.zeros(n_gt, np.int64),
        cell_dt_off=np.arange(n_gt + 1) * 10, tl_vid_start=np.zeros(1, np.int64),
        tl_image_id=np.arange(20) + 500,
        gt_frame_pos=np.concatenate([np.arange(n) for n in np.diff(t[0])]))
    ev = TaoEval.__new__(TaoEval)
    ev._run = types.SimpleNamespace(occlusion_table=occlusion_table, flat=flat, calls=calls)
    ev._occlusions, ev._cat_pos = {}, cat_pos
    ev._gt_columns = types.SimpleNamespace(ann_vis=t[1])
    ev.params = types.SimpleNamespace(cat_ids=list(cat_ids))
    return ev


def test_class_layer_on_a_stubbed_pass():
    import pytest
    ev = _stubbed()
    e = ev.occlusions(0.5, (0.0, 0.1), 2, ref.HAND_EDGES)
    assert list(e) == ["columns", "counts", "len_edges", "len_lbl", "vis_rng", "frame_thr",
                       "recover"]
    assert e["columns"] == {"counts": list(ref.COUNT_COLUMNS), "tracks": list(ref.TRACK_COLUMNS),
                            "episodes": list(ref.EPISODE_COLUMNS), "outcomes": list(ref.OUTCOMES)}
    assert e["counts"].tolist() == ref.HAND_COUNTS and e["len_lbl"] == ["1", "2", "3+"]
    assert (e["len_edges"], e["vis_rng"], e["frame_thr"], e["recover"]) \
        == ([1, 2, 3], [0.0, 0.1], 0.5, 2)
    assert ev.occlusions(0.5, [0, 0.1], 2, [1, 2, 3])["counts"] is e["counts"]     # cached
    assert ev._run.calls == [(0.5, (0.0, 0.1), 2, (1, 2, 3))]
    assert ev.occlusion_lines(0.5, (0.0, 0.1), 2, ref.HAND_EDGES) == ref.HAND_LINES
    full = ev.occlusions(0.5, (0.0, 0.1), 2, ref.HAND_EDGES, per_track=True, per_episode=True)
    assert len(ev._run.calls) == 1
    ids, tracks = full["tracks"]
    assert ids.tolist() == list(range(70, 77)) and tracks.tolist() == ref.HAND_GT_OCC
    gt_id, first, last, ep = full["episodes"]
    assert gt_id.tolist() == [70 + r[0] for r in ref.HAND_EPISODES]
    assert first.tolist() == [500 + r[1] for r in ref.HAND_EPISODES]
    assert last.tolist() == [500 + r[1] + r[2] - 1 for r in ref.HAND_EPISODES]
    # entry and after: in-cell index -> the id of row 10 g + index
    for got, r in zip(ep.tolist(), ref.HAND_EPISODES):
        ident = [1000 + 10 * r[0] + x if x >= 0 else -1 for x in (r[4], r[5])]
        assert got == list(r[:4]) + ident + list(r[6:])
    ev.occlusions(0.5, (0.0, 0.1), 3, ref.HAND_EDGES)
    assert len(ev._run.calls) == 2
    # the category axis in the caller's order
    sub = _stubbed(cat_ids=(20,), cat_pos=np.array([1]))
    assert sub.occlusions(len_edges=ref.HAND_EDGES)["counts"].tolist() == ref.HAND_COUNTS[1:]
    assert sub.occlusions(len_edges=(1, 3, 6, 11))["len_lbl"] == ["1-2", "3-5", "6-10", "11+"]
    for bad in (dict(frame_thr=0.0), dict(frame_thr=float("nan")), dict(vis_rng=(0.2, 0.1)),
                dict(vis_rng=(float("nan"), 1)), dict(recover=0), dict(recover=65),
                dict(recover=1.5), dict(len_edges=()), dict(len_edges=(2, 3)),
                dict(len_edges=(1, 3, 3)), dict(len_edges=tuple(range(1, 10))),
                dict(len_edges=(1, 2.5))):
        with pytest.raises(ValueError, match=list(bad)[0]):
            ev.occlusions(**bad)
    ev._run = None
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.occlusions()


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    assert "#define TAOAMD_TRACK_OCCLUSION_LEN %d" % _lib.TRACK_OCCLUSION_LEN in text
    assert "#define TAOAMD_TRACK_OCCLUSION_RECOVER %d" % _lib.TRACK_OCCLUSION_RECOVER in text
    lib = _lib.load()
    for name in ("taoamd_track_occlusion_workspace", "taoamd_track_occlusion_count",
                 "taoamd_track_occlusion_fill"):
        assert re.search(r"\b%s\s*\(" % name, text)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.taoamd_version() >= 109
    assert _lib.OCC_EPISODE_COLUMNS == ref.EPISODE_COLUMNS
    assert _lib.OCC_TRACK_COLUMNS == ref.TRACK_COLUMNS
    assert _lib.OCC_COUNT_COLUMNS == ref.COUNT_COLUMNS and _lib.OCC_OUTCOMES == ref.OUTCOMES


def test_abi_refusals_come_before_the_first_device_call():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    n_gt, n_gf = 70, 3000
    need = int(lib.taoamd_track_occlusion_workspace(n_gt, n_gf, 4))
    assert need >= 4 * n_gt
    for bad in ((-1, n_gf, 4), (n_gt, -1, 4), (n_gt, n_gf, 0), (n_gt, n_gf, 9)):
        assert lib.taoamd_track_occlusion_workspace(*bad) == 0, bad
    nan = float("nan")

    def calls(n_gt=n_gt, n_gf=n_gf, n_cat=7, recover=3, lo=0.0, hi=0.1, edges=(1, 3, 6, 11),
              n_len=None, cap=10, nbytes=need - 1):
        e = np.asarray(edges, dtype=np.int32)
        head = (n_gt, n_gf, n_cat, len(e) if n_len is None else n_len, recover, lo, hi,
                e.ctypes.data, p, p, p, p, p)
        return (lib.taoamd_track_occlusion_count(*head, p, p, p, p, nbytes, None),
                lib.taoamd_track_occlusion_fill(*head, p, cap, p, p, nbytes, None))
    for bad in (dict(recover=0), dict(recover=65), dict(recover=-1),
                dict(n_len=0), dict(edges=(1,) + tuple(range(2, 10))),
                dict(edges=(0, 3)), dict(edges=(2, 3)), dict(edges=(1, 3, 3)),
                dict(edges=(1, 5, 4)), dict(lo=0.2, hi=0.1), dict(lo=nan), dict(hi=nan),
                dict(n_gt=-1), dict(n_gf=-1), dict(n_cat=0)):
        assert calls(**bad) == (2, 2), bad
    assert calls(cap=-1) == (4, 2)
    # good arguments, one byte short: the workspace check, still no device call
    for good in (dict(), dict(recover=1), dict(recover=64), dict(edges=(1,)),
                 dict(edges=tuple(range(1, 9))), dict(lo=0.1, hi=0.1), dict(cap=0),
                 dict(lo=-float("inf"), hi=float("inf"))):
        assert calls(**good) == (4, 4), good
