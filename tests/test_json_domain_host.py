"""The prediction-file population of tests/jsonpop.py on the host: json.load +
the reference's column build, the host reader (csrc/ingest.cpp) and the host
build of csrc/decfloat.hpp against what the population states -- so that the
device reader (test_gpu_json_domain.py) is held to something verified."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import jsonpop
from test_decfloat import many, shim        # noqa: F401  (the host build of decfloat.hpp)
from tao_amodal_amd.columns import DTColumns

HAVE = os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                   "tao_amodal_amd", "libtao_amodal_ingest.so"))
needs_reader = pytest.mark.skipif(not HAVE, reason="ingest library not built")
FIELDS = DTColumns.FIELDS


def host(path):
    os.environ["TAOAMD_DEVICE_INGEST"] = "0"
    try:
        return DTColumns.from_file_native(path)
    finally:
        del os.environ["TAOAMD_DEVICE_INGEST"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b, rows=None, what=""):
    assert len(a) == len(b), what
    for f in FIELDS:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.dtype == y.dtype and x.shape == y.shape, (what, f)
        if rows is not None:
            x, y = x[rows], y[rows]
        assert (bits(x) == bits(y)).all(), (what, f)


def written(f, tmp_path):
    p = str(tmp_path / (f.name + ".json"))
    with open(p, "wb") as out:
        out.write(f.text)
    return p


@needs_reader
@pytest.mark.parametrize("group", list(jsonpop.GROUPS))
def test_host_reader_json_load_and_population_agree(group, tmp_path):
    for f in jsonpop.files(group):
        try:
            data = json.loads(f.text)
        except ValueError:
            data = None
        assert (data is not None) == f.json_ok, f.name
        p = written(f, tmp_path)
        if f.host_error is not None:
            with pytest.raises(Exception) as e:
                host(p)
            assert type(e.value).__name__ in f.host_error, f.name
            continue
        h = host(p)
        if f.whole_file_to_host:
            continue
        assert len(h) == f.n and len(f.starts) == f.n, f.name
        assert all(f.text[s:s + 1] == b"{" for s in f.starts), f.name
        pop = DTColumns(**f.rows)
        same(h, pop, f.decided, f.name)
        if data is not None:
            # (every object holds the four required keys: host_error is None)
            j = DTColumns.from_json(data)
            same(h, j, None, f.name)
            same(j, pop, f.decided, f.name)
        os.remove(p)


@needs_reader
def test_handed_over_objects_the_host_reader_accepts(tmp_path):
    """The variant of H the public path is tested with: json.loads and the host
    reader read every object, the same bits (NaN, true and 9.0 included)."""
    f = jsonpop.handover_valid(3 * len(jsonpop.H_VALID))
    assert len(f.flagged) == 3 * len(jsonpop.H_VALID) and f.n == 4 * len(jsonpop.H_VALID)
    h, j = host(written(f, tmp_path)), DTColumns.from_json(json.loads(f.text))
    same(h, j, None, f.name)
    same(h, DTColumns(**f.rows), f.decided, f.name)
    assert np.isnan(h.score[f.flagged[0]]) and h.score[f.flagged[3]] == 1.0


@pytest.mark.parametrize("which", ["D1", "D2", "D3", "D4", "D5"])
def test_decimal_populations_on_the_host_build(which, shim):     # noqa: F811
    strings, dealt = jsonpop.decimal_strings(which)
    assert len(strings) == {"D1": 100000, "D2": 100000, "D3": 2691, "D4": 5000, "D5": 48}[which]
    assert len(dealt) % 5 == 0 and len(dealt) - len(strings) < 5
    out, used = many(shim, strings)
    undecided = {s for s, u in zip(strings, used) if u == 0}
    assert undecided == set(jsonpop.D5_UNDECIDED if which == "D5" else ())
    ok = used > 0
    assert (used[ok] == np.array([len(s) for s in strings])[ok]).all()
    want = np.array([float(s) for s in strings])
    assert (bits(out[ok]) == bits(want[ok])).all()
    f = next(jsonpop.files(which))
    assert f.n == len(dealt) // 5 and f.flagged == [] and not f.whole_file_to_host
    assert (bits(np.column_stack([f.rows["bbox"], f.rows["score"]]).ravel())
            == bits(np.array([jsonpop.dbl(s) for s in dealt]))).all()


def test_decimal_populations_hold_what_they_claim():
    d2 = jsonpop.decimal_strings("D2")[0]
    digits = [sum(c.isdigit() for c in s.lower().split("e")[0]) for s in d2]
    assert min(digits) == 1 and max(digits) >= 19
    assert any("E+" in s for s in d2) and any("e-" in s for s in d2)
    assert 0.25 < sum(s[0] == "-" for s in d2) / len(d2) < 0.35
    d4 = jsonpop.decimal_strings("D4")[0]
    for s in d4:                      # exactly halfway between two neighbouring doubles
        v, x = Fraction(s), float(s)
        a, b = (np.nextafter(x, -np.inf), x) if Fraction(x) > v else (x, np.nextafter(x, np.inf))
        a, b = Fraction(float(a)), Fraction(float(b))
        assert a < v < b and v - a == b - v, s


def _object_texts(f):
    ends = list(f.starts[1:]) + [len(f.text)]
    return [f.text[s:e].rstrip(b" \t\r\n],") for s, e in zip(f.starts, ends)]


def _row(r):
    """The reference's row of one object (lvis_amodal/results.py, DTColumns.from_json)."""
    c = DTColumns.from_json([r])
    return tuple(bits(getattr(c, f)).tolist() for f in FIELDS)


@needs_reader
@pytest.mark.parametrize("group", ["H", "W", "K"])
def test_stated_flags_and_values_are_the_references(group, tmp_path):
    seen = not_json = 0
    for f in jsonpop.files(group):
        pop = DTColumns(**f.rows)
        for k, text in enumerate(_object_texts(f)):
            try:
                r = json.loads(text)
            except ValueError:
                # not JSON ("007"): the kernel hands it over; what then happens
                # is the host reader's business (it reads 7)
                assert k in f.flagged, (f.name, k)
                not_json += 1
                continue
            try:
                want = _row(r)
            except (KeyError, ValueError):
                # the reference's column build raises (a missing key, a box that
                # is not of four numbers): handed over, and the host reader raises
                assert k in f.flagged, (f.name, k)
                p = str(tmp_path / "one.json")
                with open(p, "wb") as out:
                    out.write(b"[" + text + b"]")
                with pytest.raises((KeyError, ValueError)):
                    host(p)
                seen += 1
                continue
            if k not in f.flagged:
                assert want == tuple(bits(getattr(pop, x)[k:k + 1]).tolist() for x in FIELDS), \
                    (f.name, k)
    assert (seen, not_json) == {"H": (4, 1), "W": (0, 0), "K": (0, 0)}[group]


def test_structure_population_holds_what_it_claims():
    at = {}
    for f in jsonpop.files("S-edges"):
        byte, off = f.name[2:].rsplit("-", 1)
        off = int(off)
        want = {"open": b"{", "close": b"}", "quote-open": b'"', "quote-close": b'"',
                "comma": b",", "end": b"]"}[byte]
        assert f.text[off:off + 1] == want, f.name
        if byte == "open":
            assert off in f.starts
        if byte.startswith("quote"):
            s = f.text.index(jsonpop.BRACKETS.encode(), off - 7)
            assert off == (s - 1 if byte == "quote-open" else s + len(jsonpop.BRACKETS))
        if byte == "end":
            assert len(f.text) == off + 1
        else:
            assert sum(s > off for s in f.starts) >= 5      # objects behind the edge
        at[(byte, off)] = f.n
    assert sorted(at) == sorted((b, B - d) for b in jsonpop.EDGE_BYTES
                                for B in (64, 4096, 16384, 32768) for d in (0, 1))
    assert [len(f.text) for f in jsonpop.files("S-lengths")] == \
        [16383, 16384, 16385, 32767, 32768, 32769]
    assert [f.n for f in jsonpop.files("S-counts")] == [0, 1, 255, 256, 257]
    long_string, deep = list(jsonpop.files("S-carried"))
    a = long_string.text.index(b'"]')
    b = long_string.text.index(b'"', a + 1)
    assert b - a - 1 == 3 * 16384 + 17 and sum(s > b for s in long_string.starts) >= 6
    assert (b // 16384) - (a // 16384) >= 3            # whole blocks inside the string
    d = deep.text
    depth = best = 0
    for c in d[:d.index(b"  ")]:
        depth += c in b"[{"
        depth -= c in b"]}"
        best = max(best, depth)
    assert best == 72                                  # the list, the object, 70 more
    assert d.count(b" " * 40960) == 1 and sum(s > d.rindex(b"  ") for s in deep.starts) >= 6
    for f in jsonpop.files("S-blocks"):
        n_blk = (len(f.text) + jsonpop.BLK - 1) // jsonpop.BLK
        assert "S-blocks-%d" % n_blk == f.name and len(f.text) <= 33 * 2 ** 20
        held = {int(s) // jsonpop.BLK for s in f.starts}
        rounds = range((n_blk + 1023) // 1024)
        assert {0, n_blk - 1} <= held
        for r in rounds:                   # the first and the last block of every round
            assert {1024 * r, min(1024 * r + 1023, n_blk - 1)} <= held, (f.name, r)
