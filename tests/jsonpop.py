"""Prediction files for the device reader (csrc/json_ingest.hip): the population
the reader's tests share (test_json_domain_host.py, test_gpu_json_domain.py).

Every file comes with what must happen to it, stated from what the generator
put in and never by parsing the text a second time:

  text                 the file's bytes
  whole_file_to_host   the device reader steps aside (TAOAMD_JSON_FALLBACK)
  n, starts            else: the objects of the list, the offset of each one's '{'
  flagged              the objects the kernel must leave to the host reader
  rows                 the six columns of every other object: doubles are
                       float(s) of the very substring written (of int(s) where
                       it is spelt as an integer, as json.load reads it: "-0"
                       is +0.0), ids int(s), an absent track_id / video_id is -1
  json_ok, host_error  json.loads' verdict, and the exception the host reader
                       (csrc/ingest.cpp) raises for the file: its type's name,
                       names where several objects are malformed, None: it reads it

Populations (GROUPS): D1-D5 decimal strings, H what the kernel hands over, W the
64-byte number window, K keys, G what stands between the objects, S the
blocking edges of the structure passes (4 bytes a word, 64 a thread, 4096 a
wavefront, 16384 a block, 1024 blocks a round of the single-workgroup scan)."""
import functools
import random
import struct

import numpy as np

BLK = 16384                 # bytes of a block of the structure passes
ROUND = 1024                # blocks of a round of the scan kernel
WINDOW = 64                 # bytes js_object hands the number parser
BRACKETS = "]}[{,:"         # what a string may hold and the walk must not read
D_OBJECTS = 20000           # objects of D1 and D2 (five strings each)


class File:
    def __init__(self, name, text, whole=False, starts=(), rows=(), json_ok=True,
                 host_error=None):
        self.name, self.text, self.whole_file_to_host = name, text, whole
        self.json_ok = json_ok
        self.host_error = (host_error,) if isinstance(host_error, str) else host_error
        self.n = 0 if whole else len(rows)
        self.starts = np.asarray(starts, np.int64)
        self.flagged = [k for k, r in enumerate(rows) if r is None]
        n = self.n
        self.rows = {"image_id": np.zeros(n, np.int64), "category_id": np.zeros(n, np.int64),
                     "bbox": np.zeros((n, 4)), "score": np.zeros(n),
                     "track_id": np.zeros(n, np.int64), "video_id": np.zeros(n, np.int64)}
        if not whole:
            for k, r in enumerate(rows):
                if r is not None:
                    for f, v in zip(FIELDS, r):
                        self.rows[f][k] = v

    @property
    def decided(self):
        m = np.ones(self.n, bool)
        m[self.flagged] = False
        return m


FIELDS = ("image_id", "category_id", "bbox", "score", "track_id", "video_id")
BOX = ("1", "2.5", "3e1", "4")


def dbl(s):
    """The double json.load + the reference's column build make of a number."""
    return float(s) if set(s) & set(".eE") else float(int(s))


def obj(k, box=BOX, score="0.5", img=None, cat="1", trk=None, vid=None, flagged=False,
        drop=(), pre="", post="", sep=", ", colon=": ", inner=("", "")):
    """One object's text and its row (None: the kernel must hand it over)."""
    img = str(k) if img is None else img
    fields = [("image_id", img), ("category_id", cat),
              ("bbox", "[" + sep.join(box) + "]"), ("score", score)]
    if trk is not None:
        fields.append(("track_id", trk))
    if vid is not None:
        fields.append(("video_id", vid))
    body = sep.join('"%s"%s%s' % (f, colon, v) for f, v in fields if f not in drop)
    text = ("{" + inner[0] + pre + body + post + inner[1] + "}").encode("utf-8")
    if flagged:
        return text, None
    return text, (int(img), int(cat), tuple(dbl(b) for b in box), dbl(score),
                  -1 if trk is None else int(trk), -1 if vid is None else int(vid))


def plain(k):
    """The filler object: every key, spellings that vary with k."""
    return obj(k, box=(str(k % 7), "2.5", "%de1" % (k % 9), "%d.25" % k),
               score="0.%03d" % (k % 1000 + 1), trk=str(3 * k) if k % 2 else None,
               vid=str(k % 5) if k % 3 else None)


def noted(k, note=BRACKETS):
    """A filler object led by an unknown key whose string value holds brackets."""
    return obj(k, pre='"note": "%s", ' % note, trk=str(k))


class Builder:
    def __init__(self, head=b"["):
        self.parts, self.len = [], 0
        self.starts, self.rows, self.k, self.need_sep = [], [], 0, False
        self.raw(head)

    def raw(self, b):
        self.parts.append(b)
        self.len += len(b)

    def pad_to(self, off, ws=b" "):
        assert off >= self.len, (off, self.len)
        self.raw(ws * (off - self.len))

    def sep(self):
        if self.need_sep:
            self.raw(b",")
            self.need_sep = False

    def obj(self, text_row, at=None, byte=0):
        """Appends an object; with `at`, byte `byte` of its text lands on offset `at`."""
        text, row = text_row
        self.sep()
        if at is not None:
            self.pad_to(at - byte)
        self.starts.append(self.len)
        self.raw(text)
        self.rows.append(row)
        self.need_sep = True
        self.k += 1

    def fill(self, off):
        """Filler objects while they end before `off` (every fourth noted)."""
        while True:
            t = noted(self.k) if self.k % 4 == 3 else plain(self.k)
            if self.len + len(t[0]) + 2 > off:
                return
            self.obj(t)
            self.raw(b"\n" if self.k % 2 else b"")

    def some(self, n):
        for _ in range(n):
            self.obj(noted(self.k) if self.k % 4 == 3 else plain(self.k))

    def finish(self, name, tail=b"]", **kw):
        self.raw(tail)
        return File(name, b"".join(self.parts), starts=self.starts, rows=self.rows, **kw)


# ------------------------------------------------------------------ decimals
def d1_strings():
    rng, out = random.Random(2041), []
    while len(out) < 5 * D_OBJECTS:
        x = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        if x == x and x not in (float("inf"), float("-inf")):
            out.append(repr(x))
    return out


def digit_string(rng):
    """tests/test_decfloat.py's digit strings: 1-19 digits, the point anywhere,
    e/E with +, - or no sign, exponents 0-340, 30 % negative."""
    nd = rng.randint(1, 19)
    digits = str(rng.randint(1, 9)) + "".join(rng.choice("0123456789") for _ in range(nd - 1))
    cut = rng.randint(0, nd)
    s = (digits[:cut] or "0") + ("." + digits[cut:] if cut < nd else "")
    if rng.random() < 0.6:
        s += rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.randint(0, 340))
    return "-" + s if rng.random() < 0.3 else s


def d2_strings():
    rng = random.Random(2042)
    return [digit_string(rng) for _ in range(5 * D_OBJECTS)]


def d3_strings():
    out = []
    for e in range(-1070, 1020, 7):
        x = 2.0 ** e
        for y in (x, np.nextafter(x, 0), np.nextafter(x, np.inf)):
            out += [repr(float(y)), "%.17e" % float(y), "%.16e" % float(y)]
    return out


def d4_strings():
    """Exact halfway cases: odd integers above 2^53, twice those, and
    2^52 + k + one half."""
    out = []
    for k in range(1667):
        out.append("%d" % (2 ** 53 + 1 + 2 * k))
    for k in range(1667):
        out.append("%d" % (2 * (2 ** 53 + 1 + 2 * k)))
    for k in range(1666):
        out.append("%d.5" % (2 ** 52 + k))
    return out


# tests/test_decfloat.py's test_edges list, and six more
D5_STRINGS = ["0", "-0", "0.0", "-0.0", "0e0", "0.000", "1", "-1", "1e22", "1e23",
              "9007199254740992", "9007199254740993", "9007199254740994",
              "9007199254740995", "4.9e-324", "5e-324", "2.4703282292062327e-324",
              "2.4703282292062328e-324", "2.2250738585072014e-308",
              "2.2250738585072011e-308", "2.225073858507201e-308",
              "1.7976931348623157e308", "1.7976931348623158e308", "1.797693134862316e308",
              "1e308", "1e309", "1e-400", "123456789012345678", "1234567890123456789",
              "0.1", "0.2", "0.30000000000000004", "1e-5", "1.5e-07", "1E5", "1e+5",
              "8.5", "0.5", "0.25", "1000000", "123.456e2", "0.000001e-300",
              "1e400", "1e-400", "-0", "-0.0", "0e5", "1E+2"]
# the strings of D5 decfloat.hpp leaves undecided (used == 0): none -- 1e400 is
# beyond DECF_Q_MAX and answered inf, 1e-400 below DECF_Q_MIN and answered 0
D5_UNDECIDED = ()

DECIMALS = {"D1": d1_strings, "D2": d2_strings, "D3": d3_strings, "D4": d4_strings,
            "D5": lambda: list(D5_STRINGS)}


@functools.lru_cache(maxsize=None)
def decimal_strings(which):
    """The population's strings, and the same padded with "1" to whole objects."""
    s = DECIMALS[which]()
    return s, s + ["1"] * (-len(s) % 5)


def decimal_file(which):
    _, s = decimal_strings(which)
    b = Builder()
    for k in range(len(s) // 5):
        und = any(x in D5_UNDECIDED for x in s[5 * k:5 * k + 5])
        b.obj(obj(k, box=tuple(s[5 * k:5 * k + 4]), score=s[5 * k + 4], flagged=und))
        b.raw(b"\n")
    return b.finish(which)


# ------------------------------------------------------------- handed over
# (spelling of the score, does json.loads + the reference read it)
H_SCORES = ["NaN", "Infinity", "-Infinity", "true", "false", "null"]
DIGITS20 = "0.12345678901234567890"
EXP5 = "1e00005"
ID19 = "1234567890123456789"
EXACT_IDS = ["999999999999999999", "-999999999999999999", "9007199254740993", "-0"]


def handover():
    """H: one object each of what the kernel hands over, between plain ones; ids
    that must NOT be handed over and come out as exact int64."""
    b = Builder()
    b.some(2)
    for s in H_SCORES:
        b.obj(obj(b.k, score=s, flagged=True))
    b.obj(plain(b.k))
    b.obj(obj(b.k, score=DIGITS20, flagged=True))
    b.obj(obj(b.k, box=("1", "12345678901234567890", "3", "4"), flagged=True))
    b.obj(obj(b.k, score=EXP5, flagged=True))
    b.obj(obj(b.k, trk="9.0", flagged=True))
    b.obj(obj(b.k, img="1e3", flagged=True))
    b.obj(obj(b.k, vid="007", flagged=True))
    b.obj(obj(b.k, trk=ID19, flagged=True))
    b.obj(obj(b.k, trk=EXACT_IDS[0], vid=EXACT_IDS[1]))
    b.obj(obj(b.k, img=EXACT_IDS[2], cat=EXACT_IDS[0], trk=EXACT_IDS[3], vid=EXACT_IDS[3]))
    b.obj(obj(b.k, drop=("score",), flagged=True))
    b.obj(obj(b.k, box=("1", "2", "3"), flagged=True))
    b.obj(obj(b.k, box=("1", "2", "3", "4", "5"), flagged=True))
    b.obj((b"{}", None))
    b.some(3)
    # ("007" is not JSON.  The host reader raises for the null score, the missing
    # key or the short box, whichever of its threads reports first)
    return b.finish("H", json_ok=False, host_error=("KeyError", "ValueError"))


# what json.loads and the host reader both read, of the kinds H hands over
H_VALID = [dict(score="NaN"), dict(score="Infinity"), dict(score="-Infinity"),
           dict(score="true"), dict(score="false"), dict(score=DIGITS20), dict(score=EXP5),
           dict(trk="9.0"), dict(img="1e3"), dict(trk=ID19)]


def handover_valid(n_flagged, name="Hv"):
    """A file of n_flagged handed-over objects that the host reader accepts,
    a plain object after every third."""
    b = Builder()
    for j in range(n_flagged):
        b.obj(obj(b.k, flagged=True, **H_VALID[j % len(H_VALID)]))
        if j % 3 == 2:
            b.obj(plain(b.k))
        b.raw(b"\n")
    return b.finish(name)


# ------------------------------------------------------------ number window
def tiny(length):
    """0.000...05 of `length` bytes: one significant digit."""
    return "0." + "0" * (length - 3) + "5"


W_LENGTHS = (62, 63, 64, 65)


def window_files():
    out = []
    for last in ("score", "box"):
        for end in W_LENGTHS:
            b = Builder()
            b.some(1)
            for length in W_LENGTHS:
                over = length >= WINDOW
                b.obj(obj(b.k, score=tiny(length), flagged=over))
                b.obj(obj(b.k, box=BOX[:3] + (tiny(length),), flagged=over))
            # the file's last object: the number, "}]" (or "]}]"), the end of the file
            if last == "score":
                b.obj(obj(b.k, score=tiny(end), flagged=end >= WINDOW))
            else:
                b.obj(obj(b.k, box=BOX[:3] + (tiny(end),), drop=("score",),
                          pre='"score": 0.5, ', flagged=end >= WINDOW))
            assert b.parts[-1].endswith(b"5}" if last == "score" else b"5]}")
            out.append(b.finish("W-%s-%d" % (last, end)))
    return out


# --------------------------------------------------------------------- keys
UTF8 = "caf\u00e9 \u00a2 \u0710 \u06c0 \u0750 \u2603 \u6771\u4eac"


def keys_file():
    b = Builder(b"\r\n\t[\t")
    b.obj(obj(b.k, pre='"scores": 9, "Score": 9, "bbox2": [9, 9, 9, 9], "image_ids": 9, '
                       '"track_id ": 9, "Image_id": 9, "video_i": 9, '))
    b.raw(b"\r\n")
    b.obj(obj(b.k, pre='"extra": {"score": 9, "image_id": "x", "bbox": [1]}, ', vid="4"))
    b.obj(obj(b.k, pre='"name": "score", ', post=', "label": "bbox", "category": "category_id"'))
    # a known key twice: the last one wins
    t, r = obj(b.k, score="0.25", trk="1", post=', "score": 0.75, "image_id": 77, '
                                                 '"bbox": [5, 6, 7, 8.5], "track_id": 2')
    b.obj((t, (77, 1, (5.0, 6.0, 7.0, 8.5), 0.75, 2, -1)))
    b.raw(b"\t\r\n")
    b.obj(obj(b.k, pre='"na\u00efve %s": "%s %s", ' % (BRACKETS, UTF8, BRACKETS),
              post=', "\u6771": "%s"' % UTF8))
    b.obj(obj(b.k, sep="\t,\r\n\t", colon="\t:\r\n", inner=("\r\n\t", "\r\n"), trk="5", vid="6"))
    b.raw(b"\r\n\t")
    b.obj(obj(b.k, pre='"score ": 9, " score": 9, "SCORE": 9, "scor": 9, '))
    b.some(2)
    return b.finish("K", tail=b"\t]\r\n")


# ------------------------------------------------------ between the objects
def between_files():
    o = [plain(k) for k in range(3)]
    t = [x[0] for x in o]
    r = [x[1] for x in o]

    def kept(name, text, rows, starts, json_ok):
        return File(name, text, starts=starts, rows=rows, json_ok=json_ok)

    def whole(name, text, json_ok, host_error):
        return File(name, text, whole=True, json_ok=json_ok, host_error=host_error)
    # commas and white space between the list's objects: the kernel reads the
    # objects, as the host reader does
    out = [kept("G-lead-comma", b"[," + t[0] + b"]", r[:1], [2], False),
           kept("G-two-commas", b"[" + t[0] + b",," + t[1] + b"]", r[:2], [1, 3 + len(t[0])],
                False),
           kept("G-no-comma", b"[" + t[0] + b" " + t[1] + b"]", r[:2], [1, 2 + len(t[0])], False),
           kept("G-trail-comma", b"[" + t[0] + b",]", r[:1], [1], False),
           # anything else: the whole file is the host reader's
           whole("G-close-twice", b"[]]", False, "ValueError"),
           whole("G-close-open", b"][", False, "AssertionError"),
           whole("G-brace-after", b"[" + t[0] + b"]{", False, "ValueError"),
           whole("G-open-after", b"[" + t[0] + b"][", False, "ValueError"),
           whole("G-string", b'"abc"', True, "AssertionError"),
           whole("G-number", b"5", True, "AssertionError"),
           whole("G-nested-list", b"[[" + t[0] + b"]]", True, "ValueError")]
    return out


# ---------------------------------------------------------- structure edges
EDGES = (64, 4096, BLK, 2 * BLK)
EDGE_BYTES = ("open", "close", "quote-open", "quote-close", "comma", "end")


def compact(k):
    """The shortest filler (57 bytes at k < 10): fits in front of offset 63."""
    return obj(k, box=("1", "2", "3", "4"), score="1", sep=",", colon=":")


def edge_file(byte, at):
    """One of EDGE_BYTES on offset `at`, filler objects before and behind."""
    b = Builder()
    name = "S-%s-%d" % (byte, at)
    if byte in ("end", "comma"):
        b.fill(at - 1)
        if not b.need_sep:
            b.obj(compact(b.k))
        b.pad_to(at)
        if byte == "end":
            return b.finish(name)
        b.sep()
    else:
        def target(k):
            t = compact(k) if byte == "close" and at < 256 else noted(k)
            return t, {"open": 0, "close": len(t[0]) - 1, "quote-open": t[0].find(b'"]'),
                       "quote-close": t[0].find(b':"') + 1}[byte]
        b.fill(at - target(10 ** 4)[1] - 1)
        t, where = target(b.k)
        b.obj(t, at=at, byte=where)
    assert b"".join(b.parts)[at:at + 1] == {"open": b"{", "close": b"}", "comma": b","}.get(
        byte, b'"')
    b.some(5)
    return b.finish(name, tail=b"\n]\n")


def long_string_file():
    """An unknown key's string of 3 blocks + 17 bytes of brackets: whole blocks
    inside a string, without a quote."""
    b = Builder()
    b.some(3)
    n = 3 * BLK + 17
    b.obj(noted(b.k, note=(BRACKETS * (n // len(BRACKETS) + 1))[:n]))
    b.some(6)
    return b.finish("S-long-string")


def deep_file():
    """An unknown key's value nested 70 deep, 40 KB of white space between the
    opening and the closing brackets: depth carried through blocks without one."""
    b = Builder()
    b.some(3)
    deep = '[{"k": ' * 35 + '"%s"' % BRACKETS + " " * 41000 + "}]" * 35
    b.obj(obj(b.k, pre='"deep": %s, ' % deep, vid="2"))
    b.some(6)
    return b.finish("S-deep")


def length_file(length):
    """A file of exactly `length` bytes, its last byte the list's ']'."""
    b = Builder()
    b.fill(length - 1)
    b.pad_to(length - 1, b"\n")
    f = b.finish("S-len-%d" % length)
    assert len(f.text) == length
    return f


def rounds_file(n_blk):
    """A file of n_blk blocks, built by padding: objects with bracket-bearing
    strings in the first and the last block of every round of the scan, and a
    string across every round's end."""
    b = Builder()
    b.some(2)
    for r in range(ROUND, n_blk + 1, ROUND):
        b.obj(plain(b.k), at=(r - 1) * BLK + 7)            # the round's last block
        if r < n_blk:
            # a string from block r - 1 into block r, the next round's first
            b.obj(noted(b.k, note=BRACKETS * 40), at=r * BLK - 100)
            assert b.len > r * BLK + 100
            b.obj(plain(b.k))
    b.obj(noted(b.k), at=n_blk * BLK - 300)
    b.pad_to(n_blk * BLK - 6)
    f = b.finish("S-blocks-%d" % n_blk)
    assert (len(f.text) + BLK - 1) // BLK == n_blk
    return f


def count_file(n):
    b = Builder()
    b.some(n)
    return b.finish("S-count-%d" % n)


S_LENGTHS = tuple(BLK * k + d for k in (1, 2) for d in (-1, 0, 1))
S_BLOCKS = (1023, 1024, 1025, 2049)
S_COUNTS = (0, 1, 255, 256, 257)

GROUPS = {
    "D1": [lambda: decimal_file("D1")], "D2": [lambda: decimal_file("D2")],
    "D3": [lambda: decimal_file("D3")], "D4": [lambda: decimal_file("D4")],
    "D5": [lambda: decimal_file("D5")],
    "H": [handover], "W": [window_files], "K": [keys_file], "G": [between_files],
    "S-edges": [functools.partial(edge_file, byte, B - d)
                for B in EDGES for byte in EDGE_BYTES for d in (1, 0)],
    "S-carried": [long_string_file, deep_file],
    "S-lengths": [functools.partial(length_file, n) for n in S_LENGTHS],
    "S-counts": [functools.partial(count_file, n) for n in S_COUNTS],
    "S-blocks": [functools.partial(rounds_file, n) for n in S_BLOCKS],
}
S_GROUPS = [g for g in GROUPS if g.startswith("S-")]


def files(group):
    """The files of a group, made one after the other (the largest is 33 MB)."""
    for make in GROUPS[group]:
        out = make()
        for f in out if isinstance(out, list) else [out]:
            yield f
