"""The device prediction reader (csrc/json_ingest.hip) held to the population of
tests/jsonpop.py (pinned on the host by test_json_domain_host.py).

read() below calls the C ABI itself and so sees what the KERNELS decided,
before DTColumns._from_file_device patches the flagged objects with the host
reader's rows: the number of objects, their offsets, exactly which objects are
handed over, and every bit of every other row."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import jsonpop
import wsguard
from tao_amodal_amd import _lib
from tao_amodal_amd.columns import DTColumns

pytestmark = pytest.mark.gpu

FIELDS = DTColumns.FIELDS
SENTINEL = -0x5A5A5A5A5A5A5A5B          # in every output cell before the call
TAIL = 8                                # sentinel cells behind flag[cap]
FLAG_BYTES = 2 << 16                    # the flag buffer json_pred_open carves


@pytest.fixture(autouse=True)
def small_files_too(monkeypatch):
    import torch  # noqa: F401  (the device path needs the runtime torch loaded)
    monkeypatch.setattr(DTColumns, "DEVICE_INGEST_MIN_BYTES", 0)


def written(f, tmp_path):
    p = str(tmp_path / (f.name + ".json"))
    if not os.path.exists(p):
        with open(p, "wb") as out:
            out.write(f.text)
    return p


def r256(x):
    return (x + 255) & ~255


def short_of_the_starts(f):
    """A workspace one byte short of the fourth carve of taoamd_json_pred_open
    (text, tables, flag buffer, then the objects' offsets) from a 256-aligned base."""
    n_blk = (len(f.text) + jsonpop.BLK - 1) // jsonpop.BLK
    return r256(n_blk * jsonpop.BLK + 64) + r256((n_blk * 6 + 8) * 4) + FLAG_BYTES + \
        r256(f.n * 8) - 1


class Read:
    pass


def read(path, flag_cap=None, work="reported", to_host=False, again=False):
    """taoamd_json_pred_workspace / _open / _count / _convert (or _read) / _close.
    work: "reported" = a guarded buffer of exactly the reported size, None = no
    workspace, an int = a guarded buffer of that many bytes."""
    import torch
    lib = _lib.load()
    size = os.path.getsize(path)
    reported = int(lib.taoamd_json_pred_workspace(size))
    guard = None
    if work is not None:
        nbytes = reported if work == "reported" else int(work)
        assert nbytes <= reported
        guard = wsguard.Guarded(nbytes)
    torch.cuda.synchronize()            # (the text is copied on streams of the library's own)
    out = Read()
    status, err = C.c_int32(-1), C.create_string_buffer(512)
    h = lib.taoamd_json_pred_open(os.fsencode(path), guard.data_ptr() if guard else None,
                                  guard.nbytes if guard else 0, C.byref(status), err, 512, None)
    out.status = status.value
    if not h:
        if guard:
            guard.check()
        out.n = None
        return out
    try:
        assert status.value == _lib.OK
        n = out.n = int(lib.taoamd_json_pred_count(h))
        cap = n if flag_cap is None else flag_cap
        flag = np.full(cap + TAIL, SENTINEL, np.int64)
        flag_at = np.full(cap + TAIL, SENTINEL, np.int64)
        n_flag = C.c_int32(-1)
        shape = {f: (n, 4) if f == "bbox" else (n,) for f in FIELDS}
        if to_host:
            cols = {f: np.full(shape[f], SENTINEL, np.int64) for f in FIELDS}
            ptr = {f: cols[f].ctypes.data for f in FIELDS}
            call = lib.taoamd_json_pred_read
        else:
            dev = {f: torch.full(shape[f], SENTINEL, dtype=torch.int64, device="cuda")
                   for f in FIELDS}
            ptr = {f: dev[f].data_ptr() for f in FIELDS}
            call = lib.taoamd_json_pred_convert
            torch.cuda.synchronize()
        args = (h, ptr["image_id"], ptr["category_id"], ptr["bbox"], ptr["score"],
                ptr["track_id"], ptr["video_id"], flag.ctypes.data, flag_at.ctypes.data, cap,
                C.byref(n_flag))
        out.rc = call(*args)
        out.n_flagged = n_flag.value
        if again:
            out.rc_again = call(*args)
        if not to_host:
            torch.cuda.synchronize()
            cols = {f: dev[f].cpu().numpy() for f in FIELDS}
        out.cols, out.flag, out.flag_at, out.cap = cols, flag, flag_at, cap
    finally:
        lib.taoamd_json_pred_close(h)
    if guard:
        guard.check()
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def hold(f, got, rows_written=True):
    """What a call with flag_cap >= the flagged objects must give for file f."""
    if f.whole_file_to_host:
        assert got.n is None and got.status == _lib.JSON_FALLBACK, (f.name, got.status)
        return 0, 0
    assert got.n == f.n and got.rc == _lib.OK, (f.name, got.n, f.n)
    k = got.n_flagged
    listed = got.flag[:min(k, got.cap)]
    assert sorted(listed.tolist()) == f.flagged and k == len(f.flagged), \
        (f.name, sorted(listed.tolist())[:10], f.flagged[:10])
    assert (got.flag_at[:k] == f.starts[listed]).all(), f.name
    assert (got.flag[k:] == SENTINEL).all() and (got.flag_at[k:] == SENTINEL).all(), f.name
    m = f.decided
    for c in FIELDS:
        x, y = bits(got.cols[c]), bits(f.rows[c])
        differ = x != y if x.ndim == 1 else (x != y).any(axis=1)
        bad = np.flatnonzero(differ & m)
        assert len(bad) == 0, (f.name, c, len(bad), int(bad[0]), x[bad[0]], y[bad[0]])
        if rows_written:
            assert (x[~m] == SENTINEL).all(), (f.name, c)      # flagged rows are not written
    return f.n - k, k


# ----------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("group", list(jsonpop.GROUPS))
def test_kernels_decide_what_the_population_states(group, tmp_path):
    decided = flagged = count = 0
    for f in jsonpop.files(group):
        d, k = hold(f, read(written(f, tmp_path)))
        decided, flagged, count = decided + d, flagged + k, count + 1
        os.remove(written(f, tmp_path))
    print("%s: %d files, %d objects decided by the kernel, %d handed over"
          % (group, count, decided, flagged))
    if group in ("D1", "D2", "D3", "D4", "D5"):
        assert flagged == 0 and decided > 0


# ------------------------------------------------------------ 2. flag capacity
def test_flag_capacity(tmp_path):
    f = next(jsonpop.files("H"))
    k = len(f.flagged)
    assert k == 17
    p = written(f, tmp_path)
    for cap in (0, 1, k, k + 1):
        got = read(p, flag_cap=cap)
        assert got.rc == _lib.OK and got.n == f.n and got.n_flagged == k, cap
        listed = got.flag[:min(k, cap)].tolist()
        assert len(set(listed)) == len(listed) and set(listed) <= set(f.flagged), cap
        assert (got.flag_at[:len(listed)] == f.starts[listed]).all(), cap
        # nothing behind flag[min(k, cap)], the tail behind flag[cap] included
        assert (got.flag[len(listed):] == SENTINEL).all(), cap
        assert (got.flag_at[len(listed):] == SENTINEL).all(), cap
        m = f.decided
        for c in FIELDS:
            assert (bits(got.cols[c])[m] == bits(f.rows[c])[m]).all(), (cap, c)
            assert (bits(got.cols[c])[~m] == SENTINEL).all(), (cap, c)


# ---------------------------------------------------------------- 3. workspace
@pytest.mark.parametrize("group", jsonpop.S_GROUPS)
@pytest.mark.parametrize("how", ["shifted", "none", "short"])
def test_workspace_carves_and_their_fallbacks(group, how, tmp_path, monkeypatch):
    """A base off alignment; no workspace at all (the text, the tables and the
    offsets from hipMalloc); a workspace that holds all but the offsets."""
    if how == "shifted":
        monkeypatch.setattr(wsguard, "SHIFT", 8)
    for f in jsonpop.files(group):
        p = written(f, tmp_path)
        work = {"shifted": "reported", "none": None, "short": short_of_the_starts(f)}[how]
        hold(f, read(p, work=work))
        os.remove(p)


# --------------------------------------------------------- 4. into host arrays
@pytest.mark.parametrize("which", ["D2", "S-count-257"])
def test_read_into_host_arrays_equals_convert(which, tmp_path):
    f = next(jsonpop.files("D2")) if which == "D2" else \
        [x for x in jsonpop.files("S-counts") if x.name == which][0]
    assert which == "D2" or f.n == 257
    p = written(f, tmp_path)
    a = read(p)
    b = read(p, to_host=True, again=True)
    hold(f, a)
    hold(f, b, rows_written=False)
    assert b.rc == _lib.OK and b.rc_again == _lib.ERR_ARG
    for c in FIELDS:
        assert (bits(a.cols[c]) == bits(b.cols[c])).all(), c
    # without a workspace (the route of a fresh process)
    c_ = read(p, to_host=True, work=None)
    hold(f, c_, rows_written=False)


# -------------------------------------------------------------- 5. public path
def host(path):
    os.environ["TAOAMD_DEVICE_INGEST"] = "0"
    try:
        return DTColumns.from_file_native(path)
    finally:
        del os.environ["TAOAMD_DEVICE_INGEST"]


def device(path):
    from tao_amodal_amd import columns
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(columns.__file__)),
                              "libtao_amodal_ingest.so"))
    return DTColumns._from_file_device(path, lib)


def same(a, b, what=""):
    assert len(a) == len(b), what
    for f in FIELDS:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.dtype == y.dtype and x.shape == y.shape, (what, f)
        assert (x.view(np.uint64) == y.view(np.uint64)).all(), (what, f)


@pytest.mark.parametrize("group", list(jsonpop.GROUPS))
def test_public_path_is_the_host_readers(group, tmp_path):
    for f in jsonpop.files(group):
        p = written(f, tmp_path)
        if f.host_error is not None:
            assert device(p) is None, f.name
            with pytest.raises(Exception) as e:
                DTColumns.from_file_native(p)
            assert type(e.value).__name__ in f.host_error, f.name
        else:
            want = host(p)
            same(DTColumns.from_file_native(p), want, f.name)
            d = device(p)
            assert (d is None) == f.whole_file_to_host, f.name
            if d is not None:
                same(d, want, f.name)
        os.remove(p)


def test_public_path_at_the_flag_capacity(tmp_path):
    cap = DTColumns.DEVICE_INGEST_FLAG_CAP
    f = jsonpop.handover_valid(cap, "Hv-cap")
    assert len(f.flagged) == cap
    p = written(f, tmp_path)
    d, want = device(p), host(p)
    assert d is not None
    same(d, want)
    same(want, DTColumns.from_json(json.loads(f.text)))
    m = f.decided
    for c in FIELDS:
        assert (bits(getattr(d, c))[m] == bits(f.rows[c])[m]).all(), c
    g = jsonpop.handover_valid(cap + 1, "Hv-cap-and-one")
    p = written(g, tmp_path)
    assert device(p) is None
    same(DTColumns.from_file_native(p), host(p))


# ---------------------------------------------------------------- 6. evaluation
def spelt(x, k):
    """x with a long mantissa and an exponent (D2's spellings): the double's
    17 or 19 significant digits as an integer, a decimal or a fraction."""
    x = float(x)
    if x == 0.0:
        return "0.0"
    if k % 4 == 0:
        return "%.18e" % x
    m, e = ("%.16e" % abs(x)).split("e")
    digits, e = m.replace(".", "").lstrip("0"), int(e) - 16
    sign = "-" if x < 0 else ""
    if k % 4 == 1:
        return "%s%sE%+d" % (sign, digits, e)
    if k % 4 == 2:
        return "%s0.000%se%d" % (sign, digits, e + len(digits) + 3)
    return "%s%s.%se-%d" % (sign, digits[:5], digits[5:], -(e + len(digits) - 5)) \
        if e + len(digits) - 5 < 0 else "%s%s.%sE%d" % (sign, digits[:5], digits[5:],
                                                        e + len(digits) - 5)


def test_evaluation_on_columns_read_from_long_spellings(tmp_path):
    import orclib
    from tao_amodal_amd import engine, flatten, flatten_dev
    from tao_amodal_amd.columns import DeviceDTColumns
    from tao_amodal_amd.synth import synth
    gt, dt = synth(seed=23, V=3, F=10, C=8, dets_per_frame=20, n_present=4)
    objs = []
    for k in range(len(dt)):
        box = ", ".join(spelt(v, k + j) for j, v in enumerate(dt.bbox[k]))
        objs.append('{"image_id": %d, "category_id": %d, "bbox": [%s], "score": %s, '
                    '"track_id": %d, "video_id": %d}'
                    % (dt.image_id[k], dt.category_id[k], box, spelt(dt.score[k], k + 1),
                       dt.track_id[k], dt.video_id[k]))
    p = str(tmp_path / "pred.json")
    with open(p, "w") as f:
        f.write("[" + ",\n".join(objs) + "]\n")
    d = DTColumns.from_file_native(p)
    assert isinstance(d, DeviceDTColumns)           # every object decided on the device
    with open(p) as f:
        want = DTColumns.from_json(json.load(f))
    same(d, want)
    same(want, dt)                                  # (the spellings round-trip)
    f = flatten.flatten_lvis(gt, want)
    fd = flatten_dev.flatten_lvis_device(gt, d, "cuda:0")
    got, ref = engine.evaluate_flat(fd, "cuda:0"), orclib.run_flat(f)
    assert np.array_equal(got["precision"], ref["precision"])
    assert np.array_equal(got["recall"], ref["recall"])
    want.track_id, _ = flatten.make_track_ids_unique(want)
    d.track_id, _ = flatten.make_track_ids_unique(d)
    f = flatten.flatten_tao(gt, want)
    fd = flatten_dev.flatten_tao_device(gt, d, "cuda:0")
    got, ref = engine.evaluate_flat(fd, "cuda:0"), orclib.run_flat(f)
    assert np.array_equal(got["precision"], ref["precision"])
    assert np.array_equal(got["recall"], ref["recall"])
