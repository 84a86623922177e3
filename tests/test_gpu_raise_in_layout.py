"""The later super-chunks' precision envelope, applied by the layout pass.

Behind a one-pass sweep taoamd_accumulate* no longer runs acc_raise_kernel: the
layout kernel raises every record on its way from val to precision.  The
separate kernel stays on the paths whose val a caller reads
(taoamd_accumulate_compact + taoamd_finalize).  Here both forms sweep the same
rows and must give the same bits, the C oracle's; the rows are built so that
the envelope of the later super-chunks decides values (checked on the CPU), in
categories on every boundary of the envelope's blocking: one super-chunk (SC),
two SCs -1 / +0 / +1 row, 8 / 9 / 16 / 17 / 32 SCs (the layout kernel's lane
groups), 65 SCs (the second 64-SC round), an empty category
between long ones, K x A rows that are no multiple of the 64-row tile, one
combo word and four, ranges without ground truth, thresholds never reached.
Reference: lvis_amodal/eval.py:339-426."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import wsguard
from tao_amodal_amd import _lib
from test_gpu_sweep_modes import _oracle_tables

gpu = pytest.mark.gpu

N_THR, N_REC = _lib.N_THR, _lib.N_REC
U64 = np.uint64
EPS = 2.220446049250313e-16


def _sc_rows():
    """Rows of a super-chunk, from the kernel's own blocking constants."""
    src = os.path.join(os.path.dirname(_lib.__file__), "csrc", "accumulate.hip")
    text = open(src).read()
    sw = int(re.search(r"^#define SWEEP_SW (\d+)", text, re.M).group(1))
    nb = int(re.search(r"^#define SWEEP_NB (\d+)", text, re.M).group(1))
    return sw * nb * 64


SC = _sc_rows()


def _sizes(name):
    if name == "edges":          # 7 categories: 42 / 140 (k, r) rows, not a multiple of 64
        return [SC, 2 * SC - 1, 2 * SC, 2 * SC + 1, 3 * SC + 7, 0, 4 * SC]
    if name.startswith("groups"):   # the layout kernel scans 64 / W rows a round: W = 8, 16, 32
        w = int(name[6:])
        return [w * SC, (w // 2 + 1) * SC - 3, 2 * SC, 0, w * SC - 1]
    if name == "round2":         # 65 SCs: the scan's second round of 64
        return [65 * SC, 5, 2 * SC + 3]
    if name == "lvis":           # 1203 x 6 rows: 113 tiles, the last one partial
        s = [(7 * k) % 4 for k in range(1203)]
        for k in range(0, 1203, 150):
            s[k] = 2 * SC + k
        s[1202] = 3 * SC - 1
        return s
    raise KeyError(name)


CASES = [("edges", 6), ("edges", 20), ("groups8", 6), ("groups16", 6), ("groups32", 6),
         ("groups16", 20), ("round2", 6), ("round2", 20), ("lvis", 6)]


@functools.lru_cache(maxsize=None)
def _case(name, n_rng):
    """Rows whose precision RISES along the score order: a category opens with
    false positives, its first SC holds a few true positives among many false
    ones, every later SC is dense with true positives.  Range r of category k
    has no ground truth where (k + r) % 4 == 3, three times the true positives
    where it is 2 (the upper recall thresholds are never reached) and about as
    many as true positives elsewhere (thresholds are crossed in every SC)."""
    rng = np.random.default_rng(17 + n_rng)
    sizes = _sizes(name)
    K, nw, n = len(sizes), (n_rng * N_THR + 63) // 64, int(sum(sizes))
    cat_off = np.zeros(K + 1, np.int32)
    np.cumsum(sizes, out=cat_off[1:])
    matched = np.zeros((n, nw), U64)
    ignored = np.zeros((n, nw), U64)
    num_gt = np.zeros((K, n_rng), np.int32)
    for k, sz in enumerate(sizes):
        a, b = int(cat_off[k]), int(cat_off[k + 1])
        pos = np.arange(sz)
        p = np.where(pos < 10, 0.0, np.where(pos < SC, 0.04, 0.9))
        for r in range(n_rng):
            kind = (k + r) % 4
            tp0 = 0
            for t in range(N_THR):
                c = r * N_THR + t
                m = rng.random(sz) < p * (1 - 0.03 * t)
                ig = rng.random(sz) < (0.1 if (k + t) % 3 else 0.0)
                bit = U64(1) << U64(c % 64)
                matched[a:b, c // 64] |= np.where(m, bit, U64(0))
                ignored[a:b, c // 64] |= np.where(ig, bit, U64(0))
                if t == 0:
                    tp0 = int((m & ~ig).sum())
            if kind == 3:
                num_gt[k, r] = 0
            elif kind == 2:
                num_gt[k, r] = 3 * tp0 + 1
            else:
                num_gt[k, r] = max(1, tp0 - int(rng.integers(0, 3)))
    want_p, want_r = _oracle_tables(cat_off, matched, ignored, num_gt)
    for arr in (cat_off, matched, ignored, num_gt, want_p, want_r):
        arr.setflags(write=False)
    return cat_off, matched, ignored, num_gt, want_p, want_r


def _raise_decides(case):
    """For every category of two or more SCs: is there a (range, threshold j)
    whose final value lies above the best tp / (n + eps) of the rows of the SC
    that emitted j -- a value only the later SCs' envelope can have supplied?
    From the rows and the oracle's table alone (IoU threshold 0)."""
    cat_off, matched, ignored, num_gt, want_p, _ = case
    K, n_rng = num_gt.shape
    rec_thrs = np.linspace(0.0, 1.0, N_REC)
    verdict = {}
    for k in range(K):
        a, b = int(cat_off[k]), int(cat_off[k + 1])
        if b - a <= SC:
            continue
        verdict[k] = False
        for r in range(n_rng):
            if num_gt[k, r] <= 0:
                continue
            c = r * N_THR
            m = (matched[a:b, c // 64] >> U64(c % 64) & U64(1)).astype(bool)
            ig = (ignored[a:b, c // 64] >> U64(c % 64) & U64(1)).astype(bool)
            tp = np.cumsum(m & ~ig).astype(np.float64)
            fp = np.cumsum(~m & ~ig).astype(np.float64)
            pr = tp / (tp + fp + EPS)
            at = np.searchsorted(tp / float(num_gt[k, r]), rec_thrs, side="left")
            for j in np.flatnonzero(at < b - a):
                s = int(at[j]) // SC
                own = pr[s * SC:(s + 1) * SC].max()
                if want_p[0, j, k, r] > own:
                    verdict[k] = True
    return verdict


@functools.lru_cache(maxsize=None)
def _assert_the_raise_matters(name, n_rng):
    verdict = _raise_decides(_case(name, n_rng))
    assert len(verdict) >= 2
    assert all(verdict.values()), [k for k, v in verdict.items() if not v]


@pytest.mark.parametrize("name,n_rng", CASES)
def test_the_inputs_make_the_raise_matter(name, n_rng):
    """A condition on the inputs (CPU, the oracle alone): a kernel that forgot
    the later SCs could not produce these tables."""
    _assert_the_raise_matters(name, n_rng)


@pytest.fixture(params=["lookback", "twopass"])
def onepass_mode(request):
    _lib.sweep_mode(request.param)
    yield request.param
    _lib.sweep_mode("auto")


class _Device:
    def __init__(self, case):
        import torch
        self.torch, self.lib, self.dev = torch, _lib.load(), "cuda:0"
        cat_off, matched, ignored, num_gt = case[:4]
        self.K, self.n_rng = num_gt.shape
        self.n, self.nw = matched.shape
        dev = self.dev
        self.d_off = torch.from_numpy(np.array(cat_off)).to(dev)
        self.d_ng = torch.from_numpy(np.array(num_gt)).to(dev)
        self.rows = torch.empty((self.n, self.nw, 2), dtype=torch.int64, device=dev)
        self.rows[:, :, 0] = torch.from_numpy(np.array(matched).view(np.int64)).to(dev)
        self.rows[:, :, 1] = torch.from_numpy(np.array(ignored).view(np.int64)).to(dev)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.hint = int(np.diff(cat_off).max())

    def _tables(self):
        t = self.torch
        prec = t.full((N_THR, N_REC, self.K, self.n_rng), 7.0, dtype=t.float64, device=self.dev)
        rec = t.full((N_THR, self.K, self.n_rng), 7.0, dtype=t.float64, device=self.dev)
        ws = wsguard.Guarded(self.lib.taoamd_accumulate_workspace(self.n, self.K, self.n_rng),
                             self.dev)
        return prec, rec, ws

    def _done(self, prec, rec, ws):
        flag = C.c_int32(7)
        _lib.check(self.lib.taoamd_accumulate_error(ws.data_ptr(), self.stream,
                                                    C.addressof(flag)), "error")
        assert flag.value == 0
        ws.check()
        return prec.cpu().numpy(), rec.cpu().numpy()

    def separate_raise(self):
        """taoamd_accumulate_compact into a caller's val (acc_raise_kernel) +
        taoamd_finalize (the plain layout kernel)"""
        t, lib = self.torch, self.lib
        prec, rec, ws = self._tables()
        val = t.full((lib.taoamd_compact_elems(self.K, self.n_rng),), 7.0, dtype=t.float64,
                     device=self.dev)
        crec = t.full((self.K * self.n_rng * N_THR,), 7.0, dtype=t.float64, device=self.dev)
        _lib.check(lib.taoamd_accumulate_compact(
            self.n, self.K, self.n_rng, self.d_off.data_ptr(), self.rows[..., 0].data_ptr(),
            self.rows[..., 1].data_ptr(), self.d_ng.data_ptr(), 0, self.K, self.hint,
            val.data_ptr(), crec.data_ptr(), ws.data_ptr(), ws.nbytes, self.stream), "compact")
        _lib.check(lib.taoamd_finalize(self.K, self.n_rng, self.d_ng.data_ptr(), val.data_ptr(),
                                       crec.data_ptr(), prec.data_ptr(), rec.data_ptr(),
                                       self.stream), "finalize")
        return self._done(prec, rec, ws)

    def in_layout(self, entry):
        """taoamd_accumulate / _prepared / _by_order_compact: the raising layout kernel"""
        lib = self.lib
        prec, rec, ws = self._tables()
        head = (self.n, self.K, self.n_rng, self.d_off.data_ptr())
        tail = (self.d_ng.data_ptr(), self.hint, prec.data_ptr(), rec.data_ptr(), ws.data_ptr(),
                ws.nbytes)
        if entry == "plain":
            _lib.check(lib.taoamd_accumulate(*head, self.rows[..., 0].data_ptr(),
                                             self.rows[..., 1].data_ptr(), *tail, self.stream),
                       "taoamd_accumulate")
        elif entry == "prepared":
            _lib.check(lib.taoamd_accumulate_prepare(*head, self.hint, ws.data_ptr(), ws.nbytes,
                                                     self.stream), "prepare")
            for _ in range(2):
                _lib.check(lib.taoamd_accumulate_prepared(*head, self.rows[..., 0].data_ptr(),
                                                          self.rows[..., 1].data_ptr(), *tail,
                                                          self.stream), "prepared")
        else:
            # compact rows, every place escaped: its row comes from the row table
            from test_gpu_compact_rows import ESCAPE
            t = self.torch
            words = t.full((max(self.n, 1),), int(ESCAPE) - (1 << 32), dtype=t.int32,
                           device=self.dev)
            order = t.arange(self.n, dtype=t.int32, device=self.dev)
            _lib.check(lib.taoamd_accumulate_by_order_compact(
                *head, order.data_ptr(), words.data_ptr(), self.rows.data_ptr(), *tail, 0,
                self.stream), "by_order_compact")
        return self._done(prec, rec, ws)


@gpu
@pytest.mark.parametrize("name,n_rng", CASES)
def test_both_forms_of_the_raise_equal_the_oracle(onepass_mode, name, n_rng):
    _assert_the_raise_matters(name, n_rng)
    case = _case(name, n_rng)
    want_p, want_r = case[4:]
    d = _Device(case)
    sep_p, sep_r = d.separate_raise()
    # (bit patterns: -0.0 and 0.0 are told apart)
    assert np.array_equal(sep_r.view(U64), want_r.view(U64)), (onepass_mode, "separate")
    assert np.array_equal(sep_p.view(U64), want_p.view(U64)), (onepass_mode, "separate")
    for entry in ("plain", "prepared") + (("compact",) if n_rng == 6 else ()):
        got_p, got_r = d.in_layout(entry)
        assert np.array_equal(got_r.view(U64), sep_r.view(U64)), (onepass_mode, entry)
        assert np.array_equal(got_p.view(U64), sep_p.view(U64)), (onepass_mode, entry)
        assert np.array_equal(got_p.view(U64), want_p.view(U64)), (onepass_mode, entry)
