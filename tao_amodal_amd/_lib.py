"""ctypes binding of the C ABI declared in include/tao_amodal_hip.h and
include/tao_amodal_ingest.h.

The two headers are the only declaration: ``SIGNATURES`` / ``INGEST_SIGNATURES``
and the constants below are read from them when this module is imported (plain
``re``, nothing but the standard library -- the module is importable without
torch and without either library).  A new entry point is declared in the
header, defined in csrc/ and called; nothing is typed in here.

The shared libraries are built in-tree by ``tao_amodal_amd/csrc/build.sh`` (or
``__graft_entry__.build()``).  There is NO fallback for the device library: if
it is missing or fails to load, importing the product path raises -- results
never come from a CPU path.
"""
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
# TAOAMD_LIBRARY: another build of the same C ABI (A/B timing of kernel
# variants on one GPU box); the default is the in-tree library
SO_PATH = os.environ.get("TAOAMD_LIBRARY") or os.path.join(HERE, "libtao_amodal_hip.so")
INGEST_SO_PATH = os.path.join(HERE, "libtao_amodal_ingest.so")


class TaoAmdError(RuntimeError):
    pass


# ---- the header reader
# Scalars by name; `void` is a return type only; `const char *` is c_char_p and
# every other pointer c_void_p (which takes ints, None, ctypes arrays and byref).
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64,
            "uint32_t": C.c_uint32, "size_t": C.c_size_t, "double": C.c_double}
_PROTOTYPE = re.compile(r"([\w\s*]+?)\b(taoamd_\w+)\s*\(([^()]*)\)\s*;")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(TAOAMD_\w+)[ \t]+(-?\d+)[ \t]*$", re.M)


def _ctype(decl, prototype):
    """ctypes type of a return type or of one parameter with its name."""
    if "*" in decl:
        words = decl.replace("*", " * ").split()
        return C.c_char_p if words[:3] == ["const", "char", "*"] and len(words) <= 4 \
            else C.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if words == ["void"]:
        return None
    if not words or words[0] not in _SCALARS or len(words) > 2 \
            or not re.fullmatch(r"\w+", words[-1]):        # (`double box[4]` is no scalar)
        raise TaoAmdError("unknown type '%s' in the prototype of %s" % (decl.strip(), prototype))
    return _SCALARS[words[0]]


def parse_header(text):
    """({name: (restype, argtypes)}, {TAOAMD_X: int}) of a header's text: every
    ``ret taoamd_name(args);`` and every ``#define TAOAMD_X <integer literal>``
    outside the comments (a #define of anything else is skipped)."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    defines = {name: int(value) for name, value in _DEFINE.findall(text)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    signatures = {}
    for ret, name, args in _PROTOTYPE.findall(text):
        args = [a for a in args.split(",") if a.strip() not in ("", "void")]
        signatures[name] = (_ctype(ret, name), [_ctype(a, name) for a in args])
    return signatures, defines


def read_header(name):
    path = os.path.join(INCLUDE, name)
    try:
        with open(path) as f:
            return parse_header(f.read())
    except OSError as e:
        raise TaoAmdError("the C ABI is declared in %s, which cannot be read (%s); "
                          "there is no second copy of it" % (path, e))


# Once per process: the device header here, since the constants below come from
# it; the ingest header, which defines none, when INGEST_SIGNATURES is first asked for.
SIGNATURES, DEFINES = read_header("tao_amodal_hip.h")


def _ingest_signatures():
    if "INGEST_SIGNATURES" not in globals():
        globals()["INGEST_SIGNATURES"] = read_header("tao_amodal_ingest.h")[0]
    return globals()["INGEST_SIGNATURES"]


def __getattr__(name):
    if name == "INGEST_SIGNATURES":
        return _ingest_signatures()
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def _define(name):
    return DEFINES["TAOAMD_" + name]


OK = _define("OK")
ERR_HIP, ERR_ARG, JSON_FALLBACK = _define("ERR_HIP"), _define("ERR_ARG"), _define("JSON_FALLBACK")
N_THR, N_REC = _define("N_THR"), _define("N_REC")
LVIS_RNG, TAO_RNG = _define("LVIS_RNG"), _define("TAO_RNG")
MAX_GT_PER_CELL = _define("MAX_GT_PER_CELL")
SEGMENT_TILE = _define("SEGMENT_TILE")
ERROR_TYPES_TILE = _define("ERROR_TYPES_TILE")
TRACK_ERROR_TYPES_TILE = _define("TRACK_ERROR_TYPES_TILE")
ERROR_TYPES = ("TP", "IGNORED", "DUP", "LOC", "CLS", "BOTH", "BKG")
ERROR_IMPACT_CHUNK = _define("ERROR_IMPACT_CHUNK")
ERROR_FIXES = ("BASE", "CLS", "LOC", "BOTH", "DUP", "BKG", "MISS", "FP", "FN")
CONFUSION_TILE = _define("CONFUSION_TILE")
CONFUSION_COLUMNS = ("cls", "both", "unheld", "adopted")
TRACK_ASSOCIATION_TILE = _define("TRACK_ASSOCIATION_TILE")
TRACK_ASSOCIATION_VIS = _define("TRACK_ASSOCIATION_VIS")
ASSOC_TRACK_COLUMNS = ("frames", "covered", "ids", "switches", "fragments", "primary",
                       "primary_frames")
ASSOC_CAT_COLUMNS = ("tracks", "frames", "covered", "ids", "switches", "fragments",
                     "mostly_tracked", "mostly_lost")
ASSOC_VIS_COLUMNS = ("frames", "covered", "primary")
TRACK_OCCLUSION_LEN = _define("TRACK_OCCLUSION_LEN")
TRACK_OCCLUSION_RECOVER = _define("TRACK_OCCLUSION_RECOVER")
OCC_OUTCOMES = ("START", "UNFOLLOWED", "END", "KEPT", "SWITCHED", "LOST")
OCC_EPISODE_COLUMNS = ("gt", "a", "n", "outcome", "entry", "after", "gap", "covered", "held")
OCC_TRACK_COLUMNS = ("episodes", "frames", "kept", "switched_lost")
OCC_COUNT_COLUMNS = ("episodes", "frames", "covered", "held", "start", "unfollowed", "end",
                     "kept", "switched", "lost", "gap")
IDENT_CAT_COLUMNS = ("gt_tracks", "gt_frames", "dt_tracks", "dt_frames", "idtp", "pairs")
TRACK_SCORE_THRS = _define("TRACK_SCORE_THRS")
HOTA_ONE = _define("HOTA_ONE")
TRACK_HOTA_ALPHAS = _define("TRACK_HOTA_ALPHAS")
HOTA_RATIOS = ("hota", "deta", "assa", "detre", "detpr", "assre", "asspr", "loca")
TRACK_CLEAR_BONUS = _define("TRACK_CLEAR_BONUS")
TRACK_CLEAR_NMAX = _define("TRACK_CLEAR_NMAX")
CLEAR_TRACK_COLUMNS = ("present", "matched", "idsw", "started")
CLEAR_CAT_COLUMNS = ("tp", "idsw", "frag", "mt", "pt", "ml", "motp_sum")
CLEAR_VIS_COLUMNS = ("frames", "matched", "idsw", "q_sum")
CLEAR_RATIOS = ("mota", "motp", "moda", "smota", "clr_re", "clr_pr", "clr_f1", "mtr", "ptr",
                "mlr")


# ---- the two libraries
def bind(cdll, table, names=None):
    """Set restype and argtypes of the functions `names` (default: all) of
    `table` on `cdll`.  A symbol the library lacks -- a build older than the
    header -- raises AttributeError naming it, and nothing is bound.  Binding
    twice sets the same values: harmless from two threads at once."""
    names = list(table) if names is None else names
    missing = [name for name in names if not hasattr(cdll, name)]
    if missing:
        raise AttributeError("%s lacks %s: it is older than its header (run "
                             "tao_amodal_amd/csrc/build.sh)" % (cdll._name, ", ".join(missing)))
    for name in names:
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = table[name]
    return cdll


_lib = None
_ingest = None


def load():
    """Load the library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64/libhsa-runtime64.  It must be the HIP
    # runtime of the process: loading ours first would map a second runtime
    # (the system one named in our DT_NEEDED) that cannot see torch's device
    # allocations ("no ROCm-capable device is detected").
    import torch  # noqa: F401
    if not os.path.exists(SO_PATH):
        raise TaoAmdError(
            "HIP extension not built: %s is missing.  Run "
            "tao_amodal_amd/csrc/build.sh (or __graft_entry__.build()).  "
            "There is no CPU fallback." % SO_PATH)
    _lib = bind(C.CDLL(SO_PATH), SIGNATURES)
    return _lib


def load_ingest(required=False):
    """libtao_amodal_ingest.so (the host-only readers, writers, masks and
    vector helpers) with every function of its header bound, opened once; None
    when it is not built -- the file absent, one that does not load, or a build
    that lacks a declared symbol.  ``required``: raise instead (callers without
    a Python statement of what they ask the library for)."""
    global _ingest
    lib = _ingest
    if lib is None:
        # (the answer is published when it is complete: a thread that arrives
        # meanwhile opens and binds a handle of its own, which is harmless, and
        # is never told "not built" by a half-made one)
        lib = False
        if os.path.exists(INGEST_SO_PATH):
            try:
                lib = bind(C.CDLL(INGEST_SO_PATH), _ingest_signatures())
            except (OSError, AttributeError):
                pass
        _ingest = lib
    if required and not lib:
        raise TaoAmdError(
            "native host library not built: %s is missing or older than its header (run "
            "tao_amodal_amd/csrc/build.sh); this call has no Python fallback" % INGEST_SO_PATH)
    return lib or None


TIMING = False     # kernel_timing(True): engine passes label their launches


def kernel_timing(on):
    """Switch the library's per-kernel event timing on / off."""
    global TIMING
    TIMING = bool(on)
    check(load().taoamd_kernel_timing_enable(int(TIMING)),
          "taoamd_kernel_timing_enable")


def kernel_timing_label(label):
    load().taoamd_kernel_timing_label(label.encode() if label else None)


def kernel_timings():
    """{kernel name: (total ms, launches)} recorded since the last call
    (synchronises with the recorded events)."""
    import numpy as np
    names = C.create_string_buffer(8192)
    ms = np.zeros(128)
    calls = np.zeros(128, dtype=np.int64)
    n = C.c_int32(0)
    check(load().taoamd_kernel_timing_collect(
        C.addressof(names), len(names), ms.ctypes.data, calls.ctypes.data, 128,
        C.addressof(n)), "taoamd_kernel_timing_collect")
    out, raw = {}, names.raw.split(b"\0")
    for k in range(n.value):
        out[raw[k].decode()] = (float(ms[k]), int(calls[k]))
    return out


def set_constants(iou_thrs=None, rec_thrs=None, visibility_rng=None, area_rng=None,
                  time_rng=None):
    """Replace the calling thread's evaluation constants (taoamd_set_thresholds,
    taoamd_set_ranges); None = the reference's default for that table."""
    import numpy as np

    def arr(a, shape):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
        return a, a.ctypes.data
    lib = load()
    i, ip = arr(iou_thrs, (N_THR,))
    r, rp = arr(rec_thrs, (N_REC,))
    check(lib.taoamd_set_thresholds(ip, rp), "taoamd_set_thresholds")
    v, vp = arr(visibility_rng, (5, 2))
    a, ap = arr(area_rng, (5, 2))
    t, tp = arr(time_rng, (4, 2))
    check(lib.taoamd_set_ranges(vp, ap, tp), "taoamd_set_ranges")


SWEEP_MODES = {"auto": -1, "chunked": 0, "lookback": 1, "twopass": 2}


def sweep_mode(mode="auto", spin_limit=0):
    """Which sweep long categories take, for the process
    (taoamd_accumulate_sweep_mode: "auto" | "chunked" | "lookback" | "twopass"),
    and the look-back's poll limit (taoamd_accumulate_spin_limit; 0 default,
    < 0 every look-back gives up at once)."""
    lib = load()
    check(lib.taoamd_accumulate_sweep_mode(SWEEP_MODES[mode]), "taoamd_accumulate_sweep_mode")
    check(lib.taoamd_accumulate_spin_limit(int(spin_limit)), "taoamd_accumulate_spin_limit")


def check(status, what):
    if status != OK:
        lib = load()
        raise TaoAmdError("%s failed: %s [%s]" % (
            what, lib.taoamd_strerror(status).decode(),
            lib.taoamd_last_error().decode()))
