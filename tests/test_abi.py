"""The C-ABI library loads on a CPU-only host and exports every symbol that
include/tao_amodal_hip.h declares (no compute calls without a GPU)."""
import os
import re

import numpy as np

from tao_amodal_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "tao_amodal_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(taoamd_[a-z_0-9]+)\s*\(", text))
    assert declared, "no declarations found"
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)


def test_ingest_header_symbols_are_exported():
    text = open(os.path.join(ROOT, "include", "tao_amodal_ingest.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(taoamd_[a-z_0-9]+)\s*\(", text))
    assert len(declared) == 37, declared
    lib = _lib.load_ingest(required=True)
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert declared == set(_lib.INGEST_SIGNATURES), declared ^ set(_lib.INGEST_SIGNATURES)


def test_thresholds_are_numpy_linspace_bit_for_bit():
    lib = _lib.load()
    a, b = np.zeros(10), np.zeros(101)
    assert lib.taoamd_thresholds_host(a.ctypes.data, b.ctypes.data) == 0
    assert np.array_equal(a, np.linspace(0.5, 0.95, 10))
    assert np.array_equal(b, np.linspace(0.0, 1.0, 101))


def test_status_strings():
    lib = _lib.load()
    assert lib.taoamd_strerror(0) == b"ok"
    assert b"workspace" in lib.taoamd_strerror(4)
    assert lib.taoamd_version() >= 100


def test_sort_plan_covers_every_category():
    """taoamd_sort_plan_host (host only): the chunks tile every category, a
    chunk's buckets and scatter tiles are consecutive, sizes agree."""
    from tao_amodal_amd import engine
    chunk, tile = 16 * _lib.SEGMENT_TILE, _lib.SEGMENT_TILE
    sizes = [0, 5, 1024, 1025, 2817, chunk, chunk + 1, 0, 2 * chunk + 3000, 352 * 3 + 1]
    cat_off = np.zeros(len(sizes) + 1, np.int32)
    np.cumsum(sizes, out=cat_off[1:])
    (chunks, split, stile, bucket), (nc, ns, nt, nb), merge = engine.sort_plan(cat_off)
    assert merge and len(chunks) == nc and len(bucket) == nb and len(stile) == nt
    at, b0, t0, splits = {}, 0, 0, []
    for i, c in enumerate(chunks):
        begin, n, bucket0, nbk, stile0, final, cat = (int(x) for x in c[:7])
        assert bucket0 == b0 and 0 < n <= chunk
        assert begin == at.get(cat, int(cat_off[cat]))
        at[cat] = begin + n
        assert nbk == (1 if n <= 1024 else -(-n // 352)) and nbk <= 128
        assert final == (sizes[cat] <= chunk)
        assert (bucket[b0:b0 + nbk] == i).all()
        if nbk > 1:
            splits.append(i)
            assert stile0 == t0
            k = -(-n // tile)
            assert (stile[t0:t0 + k] == i).all()
            t0 += k
        b0 += nbk
    assert split[:ns].tolist() == splits and b0 == nb and t0 == nt
    assert all(at.get(k, int(cat_off[k])) == cat_off[k + 1] for k in range(len(sizes)))


def test_all_in_sorted_is_the_membership_test():
    lib = _lib.load_ingest(required=True)
    rng = np.random.default_rng(3)

    def ask(keys, values):
        k = np.ascontiguousarray(keys, dtype=np.int64)
        v = np.ascontiguousarray(values, dtype=np.int64)
        return lib.taoamd_host_all_in_sorted(len(k), k.ctypes.data, len(v), v.ctypes.data)
    for span in (50, 1 << 20, 1 << 40):            # bitmap and binary-search branches
        keys = np.unique(rng.integers(-span, span, 2000))
        inside = rng.choice(keys, 100000)
        assert ask(keys, inside) == 1
        outside = inside.copy()
        missing = np.setdiff1d(np.arange(keys[0] - 2, keys[-1] + 3), keys)[:1] if span == 50 \
            else np.array([keys[-1] + 1])
        outside[77777] = missing[0]
        assert ask(keys, outside) == 0
    assert ask([], []) == 1 and ask([1], []) == 1 and ask([], [1]) == 0


def test_dense_only_entry_points_refuse_the_pair_layout():
    """`ignored == matched + 1` selects the interleaved (matched,
    ignored) pair layout in taoamd_match / taoamd_accumulate*; the entry points
    that only know dense tables must refuse that relation (before touching the
    device: this runs without a GPU) instead of scrambling rows."""
    import numpy as np
    from tao_amodal_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    base = buf.ctypes.data
    order = np.zeros(4, dtype=np.int32)
    # taoamd_gather_rows(n, n_words, src_m, src_i, stride, order, dst_m, dst_i, stream)
    assert lib.taoamd_gather_rows(4, 1, base, base + 32, 1, order.ctypes.data,
                                  base + 256, base + 256 + 8, None) == 2
    # taoamd_exchange_place(n_recv, world, n_words, rows, own_rows, own_rank, src_base,
    #                       pos, out, stream): tables of 16-byte pairs only
    i64 = np.zeros(16, dtype=np.int64)
    p = i64.ctypes.data
    assert lib.taoamd_exchange_place(4, 1, 1, base + 8, base + 8, 0, p, p, base + 256,
                                     None) == 2


def test_track_iou_plan_keeps_every_task_within_its_rows():
    """taoamd_track_iou_plan_host (host only) at GT counts whose even split
    into blocks of 32 left no row for the detection track (32, 63, 64, 96):
    every task <= 32 tracks and <= 64 pairs, every pair in exactly one task."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import fixtures
    from tao_amodal_amd import engine, flatten as fl
    from tao_amodal_amd.columns import DTColumns, GTColumns
    from test_gpu_parity import _check_plan
    gtj, predj = fixtures.rule_cells([32, 63, 64, 96, 31, 33])
    gt, dt = GTColumns.from_json(gtj), DTColumns.from_json(predj)
    dt.track_id, _ = fl.make_track_ids_unique(dt)
    f = fl.flatten_tao(gt, dt)
    assert {32, 63, 64, 96} <= set(np.diff(f.cell_gt_off).tolist())
    meta = engine.track_meta(f)[0]
    _check_plan(f, meta, *engine.track_iou_plan(f, meta))


# ---- caller-allocated workspaces: one layout function each (csrc/workspace.hpp)
_WS_N = (0, 1, 2816, 2817, 1_500_000, 21_400_000, 2 ** 31 - 1)


def _workspace_shapes():
    """(size function, arguments) of every workspace over the table of shapes."""
    for n in _WS_N:
        yield "taoamd_sort_workspace", (n,)
        yield "taoamd_sort_segments_workspace", (n,)
        yield "taoamd_flat_runs_workspace", (n,)
        for merge in (0, 1):
            yield "taoamd_sort_sampled_workspace", (n, n // 352 + 1, merge)
        yield "taoamd_rle_iou_workspace", (n, 4 * n, n // 2, 2 * n)
        yield "taoamd_track_mask_iou_workspace", (n, 4 * n, n // 2, 2 * n)
        for n_cat in (1, 100, 1203):
            for n_rng in (6, 20):
                yield "taoamd_accumulate_workspace", (n, n_cat, n_rng)
        n_dt, n_gt, n_gf = n, n // 2, min(4 * n, 2 ** 31 - 2)
        if n_dt + n_gt <= 2 ** 31 - 1:      # (the search stores hold n_dt + n_gt entries)
            for name in ("association", "identity", "hota", "clear"):
                yield "taoamd_track_%s_workspace" % name, (n_dt, n_gt, n_gf)
            yield "taoamd_track_occlusion_workspace", (n_gt, n_gf, 3)
    for n_cat in (1, 100, 1203):
        for n_rng in (6, 20):
            for world in (1, 8):
                yield "taoamd_exchange_workspace", (n_cat, n_rng, world)


# what the commit before the layout functions reported, in _workspace_shapes() order
# (the track analyses: the commit before their shared search store)
_WS_BYTES_BEFORE = {
    "taoamd_sort_workspace": [18688, 18688, 86272, 87296, 36767488, 524317440, 52613366016],
    "taoamd_sort_segments_workspace": [7168, 7168, 74752, 75776, 36551168, 521387520, 52320516096],
    "taoamd_flat_runs_workspace": [792, 792, 800, 800, 6648, 84384, 8389392],
    "taoamd_sort_sampled_workspace": [17664, 18688, 17664, 18688, 115968, 183552, 115968, 184576, 52461568, 88461824, 748281600, 1261881600, 75088725504, 126628333056],
    "taoamd_rle_iou_workspace": [256, 1024, 107264, 108032, 57000448, 813200384, 81604378880],
    "taoamd_track_mask_iou_workspace": [256, 1024, 107264, 108032, 57000448, 813200384, 81604378880],
    "taoamd_accumulate_workspace": [65792, 212224, 5869312, 20033024, 70531328, 240871168, 71424, 234752, 5874944, 20055552, 70536960, 240893696, 129280, 466432, 5932800, 20287232, 70595072, 241125376, 134912, 488960, 5938432, 20309760, 70600704, 241147904, 34263808, 136934400, 40067584, 156755456, 104729600, 377593600, 487919872, 1950625792, 493723392, 1970446592, 558385664, 2191284736, 48955980544, 195723207680, 48961783808, 195743028480, 49026446080, 195963866624],
    "taoamd_exchange_workspace": [1792, 5888, 3072, 18432, 66304, 523776, 219136, 1744640, 787456, 6295040, 2623232, 20981248],
    "taoamd_track_association_workspace": [256, 768, 231168, 231680, 123000320, 1754800384],
    "taoamd_track_occlusion_workspace": [256, 256, 5888, 5888, 3000320, 42800384],
    "taoamd_track_identity_workspace": [256, 2560, 264960, 267264, 141001472, 2011600896],
    "taoamd_track_hota_workspace": [256, 3072, 321280, 324096, 171001856, 2439601152],
    "taoamd_track_clear_workspace": [512, 7680, 681984, 689152, 363051776, 5179471616],
}


def test_workspace_sizes_never_grow():
    """The sizes are measuring runs of the layout functions: the pieces + 256
    bytes for aligning the base.  The hand-written formulas they replace added
    up to 4 KB of slack; no size may exceed what those reported."""
    lib = _lib.load()
    before = {k: list(v) for k, v in _WS_BYTES_BEFORE.items()}
    for name, args in _workspace_shapes():
        new, old = int(getattr(lib, name)(*args)), before[name].pop(0)
        assert 0 < new <= old, (name, args, new, old)
    assert not any(before.values())


def _compact_bytes(lib, p, n, n_cat, n_rng, full):
    """Smallest workspace_bytes taoamd_accumulate_compact accepts (its check
    comes first; k_begin == k_end then returns before any device work)."""
    def st(nbytes):
        return lib.taoamd_accumulate_compact(n, n_cat, n_rng, p, p, p + 8, p, 0, 0, 0, p, p,
                                             p, nbytes, None)
    assert st(full) == 0
    lo, hi = 0, full            # st(lo) == 4, st(hi) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if st(mid) == 0:
            hi = mid
        else:
            assert st(mid) == 4
            lo = mid
    return hi


def test_accumulate_workspace_holds_val_and_rec_behind_the_compact_tables():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    for n in _WS_N:
        for n_cat in (1, 100, 1203):
            for n_rng in (6, 20):
                full = int(lib.taoamd_accumulate_workspace(n, n_cat, n_rng))
                compact = _compact_bytes(lib, buf.ctypes.data, n, n_cat, n_rng, full)
                records = 8 * (int(lib.taoamd_compact_elems(n_cat, n_rng)) + n_cat * n_rng * 10)
                assert full - compact >= records, (n, n_cat, n_rng, full, compact)


def test_entry_points_refuse_a_workspace_below_the_reported_size():
    """Every entry point whose workspace check precedes its first device call
    (this runs without a GPU) answers TAOAMD_ERR_WORKSPACE to one byte less
    than the size function reports, whatever the pointers."""
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    n, K, R = 100000, 7, 6
    calls = []
    nb = int(lib.taoamd_sort_workspace(n)) - 1
    calls.append(("taoamd_sort_by_cat_score", (n, p, p, p, p, p, nb, None)))
    nb = int(lib.taoamd_sort_segments_workspace(n)) - 1
    calls.append(("taoamd_sort_segments", (n, K, p, p, 40, n, p, p, p, p, p, nb, None)))
    for max_segment, merge in ((1000, 0), (n, 1)):      # merge: longer than 16 tiles
        nb = int(lib.taoamd_sort_sampled_workspace(n, 300, merge)) - 1
        calls.append(("taoamd_sort_sampled", (n, K, p, p, 40, max_segment, p, 20, p, 5, p, 40,
                                              p, 300, p, p, p, p, nb, None)))
    nb = int(lib.taoamd_accumulate_workspace(n, K, R)) - 1
    for name in ("taoamd_accumulate", "taoamd_accumulate_chunked", "taoamd_accumulate_prepared"):
        calls.append((name, (n, K, R, p, p, p + 8, p, 0, p, p, p, nb, None)))
    for name in ("taoamd_accumulate_by_order", "taoamd_accumulate_by_order_prepared",
                 "taoamd_accumulate_by_order_chunked"):
        calls.append((name, (n, K, R, p, p, p, p + 8, p, 0, p, p, p, nb, None)))
    calls.append(("taoamd_accumulate_prepare", (n, K, R, p, 0, p, nb, None)))
    nb = int(lib.taoamd_rle_iou_workspace(50, 900, 20, 400)) - 1
    calls.append(("taoamd_rle_iou", (9, p, p, p, 50, 900, p, p, p, p, 20, 400, p, p, p, p,
                                     p, p, nb, None)))
    nb = int(lib.taoamd_track_mask_iou_workspace(50, 900, 20, 400)) - 1
    calls.append(("taoamd_track_mask_iou", (9, p, p, p, 30, p, p, 50, 900, p, p, p,
                                            p, p, 20, 400, p, p, p, 0, p, None, p, nb, None)))
    nb = int(lib.taoamd_exchange_workspace(K, R, 4)) - 1
    calls.append(("taoamd_exchange_sizes", (K, R, 4, p, p, p, nb, None)))
    calls.append(("taoamd_exchange_pack", (4 * K, R, K, 4, 1, p, p, p, p, 100, p, p, nb, 0, None)))
    calls.append(("taoamd_exchange_unpack", (4 * K, R, K, 4, p, 100, p, p, p, p, p, nb, 0, None)))
    nb = int(lib.taoamd_flat_runs_workspace(n)) - 1
    calls.append(("taoamd_flat_runs", (n, p, p, p, p, p, p, nb, None)))
    calls.append(("taoamd_flat_runs_by", (n, p, p, p, p, p, p, p, nb, None)))
    calls.append(("taoamd_flat_runs64_by", (n, p, p, p, p, p, p, p, nb, None)))
    # the track analyses: (n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames) and the tables
    n_dt, n_gt, n_gf = 1000, 70, 3000
    sizes = (n_dt, n_gt, 50, 9000, 40000, n_gf)
    nb = int(lib.taoamd_track_association_workspace(n_dt, n_gt, n_gf)) - 1
    calls.append(("taoamd_track_association", (*sizes, K, 2, 0.5, *[p] * 20, nb, None)))
    edges = np.array([1, 3, 6], dtype=np.int32)       # (read on the host: starts at 1, ascends)
    nb = int(lib.taoamd_track_occlusion_workspace(n_gt, n_gf, 3)) - 1
    occ = (n_gt, n_gf, K, 3, 3, 0.0, 0.1, edges.ctypes.data, p, p, p, p, p)
    calls.append(("taoamd_track_occlusion_count", (*occ, p, p, p, p, nb, None)))
    calls.append(("taoamd_track_occlusion_fill", (*occ, p, 10, p, p, nb, None)))
    nb = int(lib.taoamd_track_identity_workspace(n_dt, n_gt, n_gf)) - 1
    calls.append(("taoamd_track_identity_share", (*sizes, 0.5, *[p] * 11, nb, None)))
    calls.append(("taoamd_track_identity_assign", (*sizes, K, *[p] * 15, nb, None)))
    alphas = np.array([0.25, 0.5, 0.75])              # (read on the host: ascending)
    nb = int(lib.taoamd_track_hota_workspace(n_dt, n_gt, n_gf)) - 1
    calls.append(("taoamd_track_hota_align", (*sizes, *[p] * 13, nb, None)))
    calls.append(("taoamd_track_hota_match", (*sizes, 3, alphas.ctypes.data, *[p] * 18, nb, None)))
    calls.append(("taoamd_track_hota_reduce", (*sizes, K, 3, *[p] * 13, nb, None)))
    nb = int(lib.taoamd_track_clear_workspace(n_dt, n_gt, n_gf)) - 1
    cand = (n_dt, n_gt, 50, 40000, n_gf, 0.5, *[p] * 10)
    calls.append(("taoamd_track_clear_count", (*cand, p, p, p, nb, None)))
    calls.append(("taoamd_track_clear_fill", (*cand, p, 10, p, p, p, p, nb, None)))
    calls.append(("taoamd_track_clear_walk", (n_dt, n_gt, 50, n_gf, 10, *[p] * 16, nb, None)))
    calls.append(("taoamd_track_clear_reduce", (n_dt, n_gt, n_gf, 10, K, 2, *[p] * 14, nb, None)))
    for name, args in calls:
        assert getattr(lib, name)(*args) == 4, name


# ---- the binding is read from the headers (_lib.parse_header)
_FORMS = """
/* a comment with code in it: int taoamd_fake(int x); (and, commas) */
#ifdef __cplusplus
extern "C" {
#endif
#define TAOAMD_PLAIN 7   /* a trailing comment */
#define TAOAMD_PRODUCT (16 * 2816)
const char *taoamd_text(int status);
int taoamd_nothing(void);
void taoamd_close(void *handle);   /* a trailing comment */
size_t taoamd_bytes(
    int64_t n, int32_t k, uint32_t u, double x, size_t s);
int taoamd_many(const char *path, const void *const *arrays, const void **ptr,
                void **event, int *elem, char *err,
                const int64_t *counts, const unsigned char *flags);
void *taoamd_open(const int64_t n);
"""


def test_reader_handles_every_prototype_form():
    import ctypes as C
    vp = C.c_void_p
    sigs, defines = _lib.parse_header(_FORMS)
    assert sigs == {
        "taoamd_text": (C.c_char_p, [C.c_int]),
        "taoamd_nothing": (C.c_int, []),
        "taoamd_close": (None, [vp]),
        "taoamd_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_uint32, C.c_double, C.c_size_t]),
        "taoamd_many": (C.c_int, [C.c_char_p, vp, vp, vp, vp, vp, vp, vp]),
        "taoamd_open": (vp, [C.c_int64]),
    }
    assert "taoamd_fake" not in sigs
    assert defines == {"TAOAMD_PLAIN": 7}


def test_reader_refuses_an_unknown_type():
    import pytest
    for text in ("int taoamd_x(float v);", "float taoamd_x(int v);",
                 "int taoamd_x(unsigned int v);", "int taoamd_x(double box[4]);"):
        with pytest.raises(_lib.TaoAmdError, match="taoamd_x"):
            _lib.parse_header(text)


def test_constants_come_from_the_header():
    sigs, defines = _lib.read_header("tao_amodal_hip.h")
    assert defines["TAOAMD_N_THR"] == 10 == _lib.N_THR
    assert "TAOAMD_SORT_CHUNK" not in defines
    assert sigs == _lib.SIGNATURES
    import pytest
    with pytest.raises(_lib.TaoAmdError, match="no_such_header.h"):
        _lib.read_header("no_such_header.h")


def test_every_declared_function_is_bound():
    import pytest
    for lib, table in ((_lib.load(), _lib.SIGNATURES),
                       (_lib.load_ingest(required=True), _lib.INGEST_SIGNATURES)):
        for name, (restype, argtypes) in table.items():
            fn = getattr(lib, name)
            assert fn.restype is restype, name
            assert list(fn.argtypes) == argtypes, name
            if argtypes:
                with pytest.raises(TypeError):      # (refused before the call: nothing runs)
                    fn()


def test_a_stale_library_is_reported_and_not_bound(monkeypatch):
    import ctypes as C
    import pytest
    table = dict(_lib.INGEST_SIGNATURES, taoamd_not_in_this_build=(C.c_int, [C.c_int64]))
    lib = C.CDLL(_lib.INGEST_SO_PATH)
    with pytest.raises(AttributeError, match="taoamd_not_in_this_build"):
        _lib.bind(lib, table)
    assert lib.taoamd_host_lookup.argtypes is None      # nothing was bound
    assert _lib.bind(lib, table, ("taoamd_host_lookup",)) is lib
    assert len(lib.taoamd_host_lookup.argtypes) == 5
    # the loader: such a build counts as not built
    monkeypatch.setattr(_lib, "_ingest", None)
    monkeypatch.setattr(_lib, "INGEST_SIGNATURES", table)
    assert _lib.load_ingest() is None
    with pytest.raises(_lib.TaoAmdError, match="build.sh"):
        _lib.load_ingest(required=True)


def test_two_threads_loading_the_ingest_library_at_once_both_get_it(monkeypatch):
    """The CLI's two readers call the loader side by side: neither may be told
    "not built" while the other is still opening and binding the library."""
    import threading
    for _ in range(200):
        monkeypatch.setattr(_lib, "_ingest", None)
        barrier, got = threading.Barrier(2), []

        def ask():
            barrier.wait()
            got.append(_lib.load_ingest())
        threads = [threading.Thread(target=ask) for _ in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert len(got) == 2 and None not in got
        assert all(len(lib.taoamd_pred_patch.argtypes) == 12 for lib in got)


def test_a_library_that_does_not_load_counts_as_not_built(monkeypatch, tmp_path):
    bad = tmp_path / "libtao_amodal_ingest.so"
    bad.write_bytes(b"not an ELF file")
    monkeypatch.setattr(_lib, "_ingest", None)
    monkeypatch.setattr(_lib, "INGEST_SO_PATH", str(bad))
    assert _lib.load_ingest() is None


def test_the_ingest_library_is_opened_once():
    lib = _lib.load_ingest()
    assert lib is not None and _lib.load_ingest() is lib
    from tao_amodal_amd import flatten
    assert flatten._host_lib() is lib
