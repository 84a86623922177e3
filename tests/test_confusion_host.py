"""The confusion table without a GPU: the numpy restatement
(tests/confusion_ref.py) on the hand-written tables with the pairs written out
by hand and on recorded fixtures against the three invariants that tie it to
the breakdown and the impact; the C ABI's new symbols and refusals; and the
class layer on a stubbed pass."""
import os
import re
import types

import numpy as np
import pytest

import confusion_ref as ref
import error_impact_ref as imp
import error_types_ref as et
import orclib
import test_error_impact_host as hand_impact
import track_error_impact_ref as timp
from goldenio import load_inputs
from tao_amodal_amd import _lib
from tao_amodal_amd.evaluation import _core
from tao_amodal_amd.evaluation.lvis_amodal import LVISEval
from tao_amodal_amd.evaluation.tao_amodal import TaoEval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["f1", "f4", "f10"]


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def _lvis_case(f, slot=0, tb=0.1):
    gt_rng, dt_rng = orclib.ranges(f)
    _, _, mg, _ = orclib.match(f, gt_rng, dt_rng)
    out = imp.error_impact(f, mg, gt_rng, orclib.thresholds()[0], slot, tb)
    return out, ref.of_impact(f, out, 6)


def test_hand_written_breakdown_table():
    """error_types_ref.hand_flat(): d4 (CLS) and d5 (BOTH) of category 0 lie on
    the missed gt 3 of category 1; d10 (CLS) of category 1 on the held gt 4 and
    d11 (BOTH) on gt 5, both of category 0.  Ranges 0 and 3 evaluate them."""
    f, dt_at, gt_at = et.hand_flat()
    out, pairs = _lvis_case(f, tb=et.HAND_TB)
    assert pairs == {(0, 0, 1): [1, 1, 1, 1], (0, 1, 0): [1, 1, 0, 0],
                     (3, 0, 1): [1, 1, 1, 1], (3, 1, 0): [1, 1, 0, 0]}
    off, gt_cat, counts = ref.csr(pairs, 3, 6)
    assert off.tolist() == [0, 1, 2, 2] + [2] * 6 + [3, 4, 4] + [4] * 6
    assert gt_cat.tolist() == [1, 0, 1, 0] and counts[1].tolist() == [1, 1, 0, 0]


def test_hand_written_impact_table():
    """The table of the impact's host test: gE and gF of category 4 are missed
    and each linked by a CLS row of category 5 and one of category 6; category
    6 wins both (0.9 over 0.3; 0.2 over a NaN in a lower row), so the two
    `adopted` land in (6, 4) alone.  d37 (BOTH, category 8) lies on gL of 7."""
    f, dt_at, gt_at = et.make_flat(hand_impact.N_IMG, hand_impact.N_CAT, hand_impact.DETS,
                                   hand_impact.GTS)
    out, pairs = _lvis_case(f, tb=et.HAND_TB)
    want = {(0, 1): [1, 1, 1, 1], (1, 0): [1, 1, 0, 0], (5, 4): [2, 0, 2, 0],
            (6, 4): [2, 0, 2, 2], (8, 7): [0, 1, 0, 0]}
    assert pairs == {(a, c, c2): n for a in (0, 3) for (c, c2), n in want.items()}
    ref.check_invariants(pairs, hand_impact.N_CAT, 6, out["types"]["dt_counts"],
                         ref.adopted_into(f, out, 6))
    assert sum(n[ref.I_ADOPTED] for n in pairs.values()) == out["events"]["adopted"] == 6


def test_rows_outside_their_segment_or_the_tables_are_skipped():
    # category 0: rows 0-2, category 1: rows 3-4; row 2 carries category 1 in
    # the segment of 0, row 4 a category outside the table
    t = dict(n_cat=2, n_rng=1, cat_off=[0, 3, 9], score=[0.5, 0.4, 0.9, 0.3, 0.2],
             dt_cat=[0, 0, 1, 1, 2], dt_type=[4, 5, 4, 4, 4], link_other=[0, 7, 1, 1, 1],
             gt_cat=[1, 0, 5], held=[0, 0, 0])
    # row 1 links outside the table; rows 2 and 3 link gt 1 of category 0: row
    # 2 is skipped, yet as a CLS row of a category inside the table it is the
    # impact's winner, so row 3 is unheld and not adopted
    assert ref.confusion_tables(**t) == {(0, 0, 1): [1, 0, 1, 1], (0, 1, 0): [1, 0, 1, 0]}
    t["link_other"] = [2, -1, 1, 1, 1]              # gt 2: a category outside the table
    assert ref.confusion_tables(**t) == {(0, 1, 0): [1, 0, 1, 0]}
    t["dt_type"] = [7, 255, 0, 4, 4]
    assert ref.confusion_tables(**t) == {(0, 1, 0): [1, 0, 1, 1]}


def _flat(name, level, relabel):
    from tao_amodal_amd import flatten as fl
    from tao_amodal_amd.columns import DTColumns, GTColumns
    gtj, predj = load_inputs(name)
    if relabel:
        predj = ref.relabelled(gtj, predj)
    gt, dt = GTColumns.from_json(gtj), DTColumns.from_json(predj)
    if level == "lvis":
        return fl.flatten_lvis(gt, dt)
    dt.track_id, _ = fl.make_track_ids_unique(dt)
    return fl.flatten_tao(gt, dt)


def _checked(f, out, n_rng, rich):
    pairs = ref.of_impact(f, out, n_rng)
    total = [sum(n[i] for n in pairs.values()) for i in range(4)]
    assert total[ref.I_ADOPTED] == out["events"]["adopted"]
    if rich:
        # the comparison is of something: CLS pairs, and rows the impact adopts
        assert total[ref.I_CLS] > 0 and total[ref.I_ADOPTED] > 0
    ref.check_invariants(pairs, len(f.cat_ids), n_rng, out["types"]["dt_counts"],
                         ref.adopted_into(f, out, n_rng))
    return total


# the recorded fixtures hold few classification errors (CLS rows on the image
# side of f1 alone): each is also run with every third track relabelled
@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_invariants_on_the_image_side_of_the_fixtures(name, relabel):
    f = _flat(name, "lvis", relabel)
    r = orclib.run_flat(f)
    out = imp.error_impact(f, r["match_gt"], r["gt_rng"], orclib.thresholds()[0], 0, 0.1)
    total = _checked(f, out, 6, relabel or name == "f1")
    if name == "f1" and relabel:
        assert total[ref.I_CLS] > total[ref.I_UNHELD] > total[ref.I_ADOPTED]  # held ones, losers


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_invariants_on_the_track_side_of_the_fixtures(name, relabel):
    f = _flat(name, "tao", relabel)
    iou, _ = orclib.track_iou(f)
    gt_rng, dt_rng = orclib.ranges(f)
    _, _, mg, _ = orclib.match(f, gt_rng, dt_rng, iou)
    out = timp.error_impact(f, iou, mg, gt_rng, dt_rng, orclib.thresholds()[0], 0, 0.1)
    _checked(f, out, 20, relabel and name in ("f1", "f10"))


# ---------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------
def test_abi_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    assert "#define TAOAMD_CONFUSION_TILE %d" % _lib.CONFUSION_TILE in text
    assert _lib.CONFUSION_TILE * 16 <= 32768
    assert _lib.CONFUSION_COLUMNS == ref.COLUMNS
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in ("taoamd_confusion_workspace", "taoamd_confusion_count", "taoamd_confusion_fill"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.taoamd_version() >= 108
    size = lib.taoamd_confusion_workspace
    assert size(0, 0, 1, 1) > 0
    assert size(1000, 1000, 5, 1) < size(1000, 1000, 5, 6) < size(1000, 1000, 5, 20) \
        < size(1000, 100000, 5, 20) < size(1000, 100000, 5000, 20)
    assert size(1000, 1000, 5, 0) == 0 and size(1000, 1000, 5, 21) == 0
    assert size(1000, 1000, 0, 6) == 0 and size(2 ** 31, 1, 5, 6) == 0
    # 12 bytes per (range, ground truth), 4 per (range, category), three pieces
    assert size(7, 64000, 1203, 20) <= 20 * (12 * 64000 + 4 * 1203) + 4 * 256


def test_abi_refusals_come_before_any_device_call():
    lib = _lib.load()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    need = lib.taoamd_confusion_workspace(8, 8, 3, 6)
    assert 0 < need <= buf.nbytes

    def count(n_dt=8, n_gt=8, n_cat=3, n_rng=6, nbytes=need, cat_off=p, held=p, off=p):
        return lib.taoamd_confusion_count(n_dt, n_gt, n_cat, n_rng, cat_off, p, p, p, p, p,
                                          held, off, p, nbytes, None)

    def fill(n_cat=3, n_rng=6, nbytes=need, cap=4, link=p, out=p):
        return lib.taoamd_confusion_fill(8, 8, n_cat, n_rng, p, p, p, p, link, p, p, p, cap,
                                         out, p, p, nbytes, None)
    for call in (count, fill):
        assert call(nbytes=need - 1) == 4           # junk pointers: nothing was dereferenced
        assert call(n_rng=0) == 2 and call(n_rng=21) == 2 and call(n_cat=0) == 2
    assert count(n_dt=-1) == 2 and count(n_gt=2 ** 31) == 2
    assert count(cat_off=None) == 2 and count(held=None) == 2 and count(off=None) == 2
    assert fill(cap=-1) == 2 and fill(link=None) == 2 and fill(out=None) == 2
    # the workspace of 20 ranges is asked for at 20 ranges
    assert count(n_rng=20) == 4 and fill(n_rng=20) == 4


# ---------------------------------------------------------------------------
# the class layer on a stubbed pass
# ---------------------------------------------------------------------------
THRS = np.linspace(0.5, 0.95, 10)
# table categories 0..4 carry the ids 10, 20, 30, 40, 50; (range, dt_cat, gt_cat) sorted
TABLE = (np.array([0, 0, 0, 0, 0, 1, 1], np.int32),
         np.array([0, 1, 1, 2, 4, 1, 3], np.int64),
         np.array([1, 0, 4, 1, 0, 0, 4], np.int64),
         np.array([[5, 1, 3, 2], [5, 0, 3, 2], [9, 2, 4, 3], [1, 0, 0, 0], [7, 7, 7, 1],
                   [2, 0, 1, 1], [0, 6, 0, 0]], np.int64), 5)
NAMES = {10: {"id": 10, "name": "bus"}, 20: {"id": 20, "name": "truck"}, 30: {"id": 30},
         40: {"id": 40, "name": "van"}, 50: {"id": 50, "name": "pickup truck"}}


class _Run:
    def __init__(self):
        self.calls = []

    def confusion_table(self, thr_index, bg_thr):
        self.calls.append((thr_index, bg_thr))
        return TABLE


def _stubbed(cls, cat_ids=(10, 20, 30, 40, 50), cat_pos=None):
    ev = cls.__new__(cls)
    ev._run, ev._confusion, ev._cat_pos = _Run(), {}, cat_pos
    gt = types.SimpleNamespace(cats=NAMES)
    if cls is LVISEval:
        ev.lvis_gt = gt
        ev.params = types.SimpleNamespace(iou_thrs=THRS, cat_ids=list(cat_ids),
                                          visibility_rng_lbl=["all"])
    else:
        ev.tao_gt = gt
        ev.params = types.SimpleNamespace(iou_thrs=THRS, cat_ids=list(cat_ids),
                                          area_rng=[0, 1], time_rng=[0], area_rng_lbl=["all"],
                                          time_rng_lbl=["all"])
    return ev


@pytest.mark.parametrize("cls", [LVISEval, TaoEval])
def test_confusion_returns_ids_and_caches(cls):
    ev = _stubbed(cls)
    e = ev.confusion(0.75, 0.25)
    assert list(e) == ["columns", "rng_lbl", "rng", "dt_cat", "gt_cat", "counts"]
    assert e["columns"] == ["cls", "both", "unheld", "adopted"]
    assert e["rng_lbl"] == (["all"] if cls is LVISEval else [("all", "all"), ("1", "all")])
    assert e["rng"].dtype == np.int32 and e["rng"].tolist() == TABLE[0].tolist()
    assert e["dt_cat"].dtype == e["gt_cat"].dtype == e["counts"].dtype == np.int64
    assert e["dt_cat"].tolist() == [10, 20, 20, 30, 50, 20, 40]
    assert e["gt_cat"].tolist() == [20, 10, 50, 20, 10, 10, 50]
    assert np.array_equal(e["counts"], TABLE[3])
    assert ev.confusion(0.75, 0.25)["counts"] is e["counts"]
    assert ev._run.calls == [(5, 0.25)]
    ev.confusion(0.5)
    assert ev._run.calls == [(5, 0.25), (0, 0.1)]
    with pytest.raises(ValueError, match="bg_thr"):
        ev.confusion(0.5, 0.5)
    ev._run = None
    with pytest.raises(RuntimeError, match=r"Please run evaluate\(\) first\."):
        ev.confusion(0.5)


def test_confusion_under_a_permuted_subset_of_categories():
    """params.cat_ids = [50, 10, 20]: table categories 4, 0, 1; the pairs with
    30 or 40 go, the others come by (range, place of dt_cat, place of gt_cat)."""
    ev = _stubbed(LVISEval, cat_ids=(50, 10, 20), cat_pos=np.array([4, 0, 1]))
    e = ev.confusion(0.5, 0.1)
    assert e["rng"].tolist() == [0, 0, 0, 0, 1]
    assert e["dt_cat"].tolist() == [50, 10, 20, 20, 20]
    assert e["gt_cat"].tolist() == [10, 20, 50, 10, 10]
    assert e["counts"][:, 0].tolist() == [7, 5, 9, 5, 2]
    m = ev.confusion_matrix(0.5, 0.1, rng=0, column="unheld")
    assert m.tolist() == [[0, 7, 0], [0, 0, 3], [4, 3, 0]]


def test_confusion_matrix_is_the_hand_table():
    ev = _stubbed(TaoEval)
    m = ev.confusion_matrix(0.5, 0.1)
    assert m.dtype == np.int64 and m.tolist() == [
        [0, 5, 0, 0, 0], [5, 0, 0, 0, 9], [0, 1, 0, 0, 0], [0, 0, 0, 0, 0], [7, 0, 0, 0, 0]]
    assert (np.diag(m) == 0).all()
    both1 = ev.confusion_matrix(0.5, 0.1, rng=1, column="both")
    assert both1.sum() == 6 and both1[3, 4] == 6
    assert ev.confusion_matrix(0.5, 0.1, rng=7).sum() == 0
    for col in ev.confusion(0.5)["columns"]:
        for a in (0, 1):
            e = ev.confusion(0.5)
            assert ev.confusion_matrix(0.5, 0.1, a, col).sum() == \
                e["counts"][e["rng"] == a, e["columns"].index(col)].sum()
    with pytest.raises(ValueError, match="column"):
        ev.confusion_matrix(0.5, 0.1, column="CLS")


HEAD = "      id predicted          id ground truth      cls     both   unheld  adopted"


def test_image_level_lines_are_the_recorded_ones():
    """adopted 3, then the two pairs of adopted 2 and cls 5 by their ids, then
    adopted 1, then 0; category 30 has no name and goes by its id."""
    ev = _stubbed(LVISEval)
    assert ev.confusion_lines(0.75, 0.25) == [
        " confusion @[ IoU=0.75 | bg=0.25 | rng=all ]",
        " " + HEAD,
        "       20 truck              50 pickup truck        9        2        4        3",
        "       10 bus                20 truck               5        1        3        2",
        "       20 truck              10 bus                 5        0        3        2",
        "       50 pickup truck       10 bus                 7        7        7        1",
        "       30 30                 20 truck               1        0        0        0"]
    # (the name columns are as wide as the names shown)
    full = ev.confusion_lines(0.75, 0.25)
    assert [x.split() for x in ev.confusion_lines(0.75, 0.25, top=2)] == \
        [x.split() for x in full[:4]]
    assert ev.confusion_lines(0.75, 0.25, top=0) == [
        full[0], "       id predicted       id ground truth      cls     both   unheld  adopted"]
    # a range past the labels goes by its index, as in the other tables
    assert ev.confusion_lines(0.5, 0.1, rng=1) == [
        " confusion @[ IoU=0.50 | bg=0.10 | rng=1 ]",
        "       id predicted       id ground truth      cls     both   unheld  adopted",
        "       20 truck           10 bus                 2        0        1        1",
        "       40 van             50 pickup truck        0        6        0        0"]


def test_track_level_lines_are_the_recorded_ones():
    ev = _stubbed(TaoEval)
    lines = ev.confusion_lines(0.75, 0.25)
    assert lines[0] == " track confusion @[ IoU=0.75 | bg=0.25 | rng=all/all ]"
    assert lines[1] == " " + HEAD and len(lines) == 7
    assert lines[1:] == _stubbed(LVISEval).confusion_lines(0.75, 0.25)[1:]
    assert ev.confusion_lines(0.5, 0.1, rng=1)[0] == \
        " track confusion @[ IoU=0.50 | bg=0.10 | rng=1/all ]"


def test_kernel_range_slots_go_to_the_callers_ranges(monkeypatch):
    """GpuRun.confusion_table on a stubbed stage: three caller ranges held by
    the kernel slots 1, 0 and 5 (in that order); what the slots 2-4 hold goes."""
    import torch
    K, n_rng = 2, 6
    # CSR over (slot, c): slot 0: (0 -> 1) ; slot 1: (1 -> 0); slot 3: (0 -> 1); slot 5: both rows
    off = np.zeros(n_rng * K + 1, np.int64)
    rows = [0 * K + 0, 1 * K + 1, 3 * K + 0, 5 * K + 0, 5 * K + 1]
    for r in rows:
        off[r + 1:] += 1
    ws = types.SimpleNamespace(conf_n=5, conf_off=torch.from_numpy(off),
                               conf_gt_cat=torch.tensor([1, 0, 1, 1, 0, 9], dtype=torch.int32),
                               conf_counts=torch.arange(24, dtype=torch.int32).reshape(6, 4))
    run = _core.GpuRun.__new__(_core.GpuRun)
    staged = []
    run.engine = types.SimpleNamespace(stage_confusion=lambda *a: staged.append(a))
    run.torch = types.SimpleNamespace(cuda=types.SimpleNamespace(synchronize=lambda d: None))
    run.dp, run.ws, run.device = types.SimpleNamespace(n_cat=K), ws, None
    c = types.SimpleNamespace(default=True, rng_blocks=[({}, [(0, 1), (1, 0), (5, 2)])])
    monkeypatch.setattr(run, "_error_pass_at", lambda thr_index: (c, 7))
    rng, dt_cat, gt_cat, counts, k = run.confusion_table(3, 0.25)
    assert staged == [(run.dp, ws, 7, 0.25)] and k == K
    assert rng.dtype == np.int32 and rng.tolist() == [0, 1, 2, 2]
    assert dt_cat.tolist() == [1, 0, 0, 1] and gt_cat.tolist() == [0, 1, 1, 0]
    assert counts[:, 0].tolist() == [4, 0, 12, 16] and counts.dtype == np.int64
    # default constants: the slots are the ranges
    monkeypatch.setattr(run, "_error_pass_at", lambda thr_index: (None, 0))
    rng, dt_cat, gt_cat, counts, _ = run.confusion_table(0, 0.1)
    assert rng.tolist() == [0, 1, 3, 5, 5] and gt_cat.tolist() == [1, 0, 1, 1, 0]


def test_multi_gpu_refusal_comes_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the refusal comes before the library is loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    from tao_amodal_amd.evaluation._dist import DistRun
    with pytest.raises(NotImplementedError, match=r"error_types\(\) in a multi-GPU run"):
        DistRun.__new__(DistRun).confusion_table(0, 0.1)
    ev = _stubbed(LVISEval)
    ev._run = DistRun.__new__(DistRun)
    with pytest.raises(NotImplementedError, match=r"error_types\(\) in a multi-GPU run"):
        ev.confusion(0.5, 0.1)
    assert ev._confusion == {}


def test_stage_refuses_masks_ahead_of_the_library(monkeypatch):
    from tao_amodal_amd import engine

    def no_library():
        raise AssertionError("the refusal comes before the library is loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    for kind, words in (("lvis", "the error breakdown is the image level's, on boxes"),
                        ("tao", "the track-level error breakdown is the track level's, on boxes")):
        dp = types.SimpleNamespace(kind=kind, mask_iou=True, iou_mode=0,
                                   cell_unit_host=np.zeros(1, np.int64))
        with pytest.raises(_lib.TaoAmdError) as err:
            engine.stage_confusion(dp, None, 0, 0.1)
        assert str(err.value) == words
