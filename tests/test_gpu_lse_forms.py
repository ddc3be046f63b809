"""GPU: every form of the full-vocabulary normaliser and of the T projection, launched the way the decode launches them.

The chain is the one full_lse_pack / full_lse_run (csrc/jlm_decode.hip) launch: jlm_pack_t_mixed(6) of the live rows, the normaliser, then
jlm_lse_combine.  The form a launch runs is the library's own answer (ABI 12: jlm_vocab_lse_mixed_form, jlm_vocab_lse_split_form,
jlm_gemm_nt_split_form); each case asserts it against the restatement in tests/fake_hip.py and against the form the case is meant for, so
a forced setting that falls through fails.  A case is (layout, row format, entry point, row bound, device count, logit regime):

* layouts: D-softmax* [200, 100, 52], [252] and [4, 36] (generic), tied [256], [128, 64] (external biases), [512]; the split launch on
  [200, 100, 52] and [32, 16, 8]; the four hybrid forms of test_vocab_lse_hybrid; the f32 stationary kernel.  V = 2 011: a ragged last tile
  whatever the tile;
* row bounds 40, 300, 2 560, 5 200 (several row tiles) and 20 480 at V = 50 k for the default-launched forms (checked on sampled rows);
* device counts 0, 1, 31-33, 127-129, 255-257 (those below the bound), bound - 1, bound, bound + 7 (clamped) and n_dev = NULL;
* logits: Gaussian (as the kernel tests); peaked -- each row's top word at 22-25 nats, 10-20 nats above its runner-up, the top word
  walking over the first and last word of every segment of k >= 32, both sides of every 32-word edge counted from the segment's first word
  (so of every tile edge, column cut and hybrid head slice) and the last ragged tile; shifted through b2 to |log Z| log2(e) ~ 39 (the loader's admission bound for the fixed-reference forms,
  FIXED_REF_MAX_BITS = 40) and past the f32 range (largest base-2 logit above 128).

Every case checks lse of the live rows against logsumexp in float64 of the same f32 operands (mixed / hybrid / stationary: 2e-6 x
max(1, |ref|); split: the bars of test_vocab_lse_split; peaked rows on the int8 / mx6 forms that miss 2e-6: see PEAKED_MISS), that `part` -- NaN-filled, with guard slices and guard rows -- is untouched
outside the live rows of the slices the launch wrote, and that lse of every row not listed or past the count is untouched.  Past the f32
range the fixed-reference forms must return a non-finite lse, never a finite wrong one.

Forced forms: test_gpu_kernels.py::test_vocab_lse_forced_forms runs this module in a child per setting."""
import ctypes
import json
import os
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                                    # noqa: E402
from jlm_amd.rowformats import LOG2E, mixed_exponents, plane_scale                           # noqa: E402
from tests.fake_hip import FakeLib, MX_FORM, MX_FORMS, T_FORMS, _atoi_env                   # noqa: E402
from tests.test_gpu_kernels import _pack, _pack_t, _split_segments, _st                     # noqa: E402

pytestmark = pytest.mark.gpu

V = 2011
BOUNDS = (40, 300, 2560, 5200)
BIG = 20480                                   # with V = 50 000, the default-launched forms, sampled rows
N_SAMPLE = 384
MAXP = 96
GUARD_SLICES, GUARD_ROWS = 3, 11
NAN_BITS = np.uint32(0x7FC00000)
LSE_SENTINEL = -1234.5
OUT = os.environ.get("JLM_LSE_FORMS_OUT")     # set for the children of the forced-form tests: one JSON line per case
FK = FakeLib()

MIXED_LAYOUTS = {"dsoftmax": [200, 100, 52], "g252": [252], "g4_36": [4, 36], "tied": [256], "xb128_64": [128, 64], "k512": [512]}
SPLIT_LAYOUTS = {"dsoftmax": [200, 100, 52], "s32_16_8": [32, 16, 8]}
HYBRID = {"tail-split": ((0, 1), None), "head-256": ((0, 1, 2), [256, 0, 0]), "first-split": ((1, 2), None), "heads": ((0, 1, 2), [128, 384, 0])}
# the kernel each mixed layout hosts by default (include/jlm_hip.h ids), per row format and entry point
DEFAULT_FORM = {("dsoftmax", "int8", 0): "MX_KERNEL_DSOFTMAX", ("dsoftmax", "int8", 1): "MX_KERNEL_DSOFTMAX",
                ("g252", "int8", 0): "MX_KERNEL_GENERIC", ("g252", "int8", 1): "MX_KERNEL_GENERIC",
                ("g4_36", "int8", 0): "MX_KERNEL_GENERIC", ("g4_36", "int8", 1): "MX_KERNEL_GENERIC",
                ("tied", "int8", 0): "MXW_KERNEL_TIED", ("tied", "int8", 1): "MXW_KERNEL_TIED_FR",
                ("xb128_64", "int8", 0): "MX_KERNEL_GENERIC_XB", ("xb128_64", "int8", 1): "MX_KERNEL_GENERIC_XB",
                ("k512", "int8", 0): "MXW_KERNEL_K512", ("k512", "int8", 1): "MXW_KERNEL_K512_FR",
                ("dsoftmax", "mx6", 0): "MX6_KERNEL_DSOFTMAX", ("dsoftmax", "mx6", 1): "MX6_KERNEL_DSOFTMAX_FR",
                ("g252", "mx6", 0): "MX6_KERNEL_GENERIC", ("g252", "mx6", 1): "MX6_KERNEL_GENERIC",
                ("g4_36", "mx6", 0): "MX6_KERNEL_GENERIC", ("g4_36", "mx6", 1): "MX6_KERNEL_GENERIC",
                ("tied", "mx6", 0): "MX6W_KERNEL_TIED", ("tied", "mx6", 1): "MX6W_KERNEL_TIED_FR",
                ("xb128_64", "mx6", 0): "MX6_KERNEL_GENERIC_XB", ("xb128_64", "mx6", 1): "MX6_KERNEL_GENERIC_XB"}
FIXED_REF_FORMS = {"MXW_KERNEL_K512_FR", "MXW_KERNEL_TIED_FR", "MX6_KERNEL_DSOFTMAX_FR", "MX6_KERNEL_TIED_FR", "MX6W_KERNEL_DSOFTMAX_FR",
                   "MX6W_KERNEL_TIED_FR"}


def _env():
    return {"mx_wide": _atoi_env("JLM_MX_WIDE", -1), "mx6_wide": _atoi_env("JLM_MX6_WIDE", -1), "waves": _atoi_env("JLM_LSE_WAVES", 8),
            "stages": _atoi_env("JLM_T_STAGES", 3), "xcd": _atoi_env("JLM_T_XCD", 1)}


def expected_mixed_form(layout, fmt, fr, env):
    """the kernel a mixed launch must run under the process's settings, spelled out (tests/test_lse_dispatch_cpu.py pins the same table)"""
    name = DEFAULT_FORM[(layout, fmt, fr)]
    if fmt == "int8":
        if layout == "dsoftmax" and env["mx_wide"] > 0:
            name = "MXW_KERNEL_DSOFTMAX"
        if layout == "tied" and env["mx_wide"] == 0:
            name = "MX_KERNEL_TIED"
    else:
        if layout == "dsoftmax" and env["mx6_wide"] > 0:
            name = "MX6W_KERNEL_DSOFTMAX_FR" if fr else "MX6W_KERNEL_DSOFTMAX"
        if layout == "tied" and env["mx6_wide"] == 0:
            name = "MX6_KERNEL_TIED_FR" if fr else "MX6_KERNEL_TIED"
    return name


def _counts(bound):
    c = [n for n in (0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257) if n < bound]
    c += [n for n in (bound - 1, bound) if n not in c]
    return c + [bound + 7, None]


def _live(bound, n):
    return bound if n is None else min(n, bound)


# ---------------------------------------------------------------------------------------------------------------- operands
class Problem:
    """operands of one (widths, bound, regime): f32 T rows, vocabulary blocks and b2 on the host and the device, the f64 log-normaliser of
    the bound's rows (or a sample of them), a row list that scatters the bound's rows over a store twice as large"""

    def __init__(self, widths, bound, regime, vocab=V, seed=0):
        rng = np.random.default_rng(zlib.crc32(repr((widths, bound, regime, vocab, seed)).encode()))
        self.widths, self.bound, self.regime, self.V = list(widths), bound, regime, vocab
        n = len(widths)
        self.cut = [vocab * i // n for i in range(n + 1)] if n > 1 else [0, vocab]
        if widths == [200, 100, 52] and vocab > 5000:
            self.cut = [0, vocab * 24 // 100, vocab * 60 // 100, vocab]
        self.t_off = [int(x) for x in np.cumsum([0] + self.widths[:-1])]
        self.ldt = int(sum(widths)) + 8
        G = 2 * bound + 9
        self.G = G
        self.rows = (G - 1 - rng.permutation(bound + 3)[:bound]).astype(np.int32)
        Bs = [(rng.standard_normal((self.cut[i + 1] - self.cut[i], k)) * 0.08).astype(np.float32) for i, k in enumerate(widths)]
        b2 = (rng.standard_normal(vocab) * 0.3).astype(np.float32)
        T = (np.tanh(rng.standard_normal((G, self.ldt))) * rng.uniform(0.05, 1.0, size=(G, 1))).astype(np.float32)
        self.top = None
        if regime == "peaked":
            # each row's top word: the first / last word of a segment, both sides of every 32-word edge counted from the segment's first
            # word -- the vocabulary tiles (32 x 1, 2, 4 or 8 words on mixed rows, 64 or 128 on split rows), so every column cut, and the
            # hybrid head slices (multiples of 128 words) start there -- and the first and last word of the segment's last 256-word tile
            # (ragged at V = 2 011 whatever the tile).  In the segments of k >= 32 only: a 22-nat logit from a handful of products would
            # need T values of ~100.
            edges = set()
            for i in range(n):
                if widths[i] < 32:
                    continue
                v0, v1 = self.cut[i], self.cut[i + 1]
                edges.update((v0, v1 - 1, v0 + 256 * ((v1 - v0 - 1) // 256)))
                edges.update(w for j in range(1, (v1 - v0 + 31) // 32) for w in (v0 + 32 * j - 1, v0 + 32 * j))
            words = np.array(sorted(edges), dtype=np.int64)
            self.top = words[np.arange(bound) % len(words)]
            for i in range(n):                                   # the words that will carry a peak: 1.5 x the norm of the others
                w = self.top[(self.top >= self.cut[i]) & (self.top < self.cut[i + 1])] - self.cut[i]
                Bs[i][np.unique(w)] *= np.float32(1.5)
            for r, w in enumerate(self.top):
                g = self.rows[r]
                i = int(np.searchsorted(self.cut, w, side="right") - 1)
                bw = Bs[i][w - self.cut[i]].astype(np.float64)
                amp = rng.uniform(22.0, 25.0)
                T[g] *= np.float32(0.05)
                T[g, self.t_off[i]:self.t_off[i] + widths[i]] = (amp * bw / (bw @ bw)).astype(np.float32)
        self.Bs, self.b2, self.T = Bs, b2, T
        if regime in ("shift39", "shift_beyond"):
            ref0 = self._ref(self.rows)
            # |log Z| log2(e) = 39 at the row with the largest |log Z| / largest base-2 logit 132 at every row's max
            if regime == "shift39":
                c = 39.0 / LOG2E - float(ref0.max())
            else:
                c = 132.0 / LOG2E - float(self._ymax(self.rows).min())
            self.b2 = (b2 + np.float32(c)).astype(np.float32)
        self.sample = np.arange(bound) if bound <= 5200 else np.sort(np.random.default_rng(bound).choice(bound, N_SAMPLE, replace=False))
        self.ref = self._ref(self.rows[self.sample])
        self.Tg = torch.as_tensor(self.T).cuda()
        self.b2g = torch.as_tensor(self.b2).cuda()
        self.rows_g = torch.as_tensor(self.rows).cuda()
        self.Bg = [torch.as_tensor(B).cuda() for B in self.Bs]

    def _y(self, rows):
        T = self.T[rows].astype(np.float64)
        return np.concatenate([T[:, self.t_off[i]:self.t_off[i] + k] @ self.Bs[i].astype(np.float64).T for i, k in enumerate(self.widths)],
                              axis=1) + self.b2.astype(np.float64)

    def _ymax(self, rows):
        return np.concatenate([self._y(rows[j:j + 512]).max(axis=1) for j in range(0, len(rows), 512)])

    def _ref(self, rows):
        out = []
        for j in range(0, len(rows), 512):
            y = self._y(rows[j:j + 512])
            m = y.max(axis=1)
            out.append(m + np.log(np.exp(y - m[:, None]).sum(axis=1)))
        return np.concatenate(out)


_PROBLEMS = {}


def problem(widths, bound, regime, vocab=V):
    key = (tuple(widths), bound, regime, vocab)
    if key not in _PROBLEMS:
        if len(_PROBLEMS) > 24:
            _PROBLEMS.clear()
        _PROBLEMS[key] = Problem(widths, bound, regime, vocab)
    return _PROBLEMS[key]


def _mixed_rows(L, P, fmt):
    """mixed rows of every segment scaled as DeviceModel._build_mixed scales them (jlm_amd/rowformats.py): 2^eB puts max(|B|, |b2| log2 e) at <= 2^14, s8 the
    power of two at or above max |f16(B 2^eB)| / 127, 2^eT puts the segment's largest |T| log2 e at <= 2^15; mx6 rows: eT + eB = 0,
    balanced between the two operands (descale 1: the fixed-reference forms run)"""
    n = len(P.widths)
    segs = (_lib.Segment * n)()
    ts, ds, s8 = (ctypes.c_float * n)(), (ctypes.c_float * n)(), (ctypes.c_float * n)()
    keep = []
    for i, k in enumerate(P.widths):
        nv, B = P.cut[i + 1] - P.cut[i], P.Bs[i]
        b2max = float(np.abs(P.b2[P.cut[i]:P.cut[i + 1]]).max()) if k % 32 else None       # (a full last block: the biases travel apart)
        tb = max(float(np.abs(P.T[:, P.t_off[i]:P.t_off[i] + k]).max()), 1.0)
        eB, eT_i = mixed_exponents(fmt, float(np.abs(B).max()), b2max, tb)
        s_b = plane_scale(fmt, float(np.abs((B * np.float32(2.0 ** eB)).astype(np.float16).astype(np.float32)).max()))
        nb = k // 32 if k % 32 == 0 else (k + 2 + 31) // 32
        dst = torch.zeros((nv, 32 * nb), dtype=torch.float32, device="cuda")
        assert L.jlm_pack_mixed(P.Bg[i].data_ptr(), nv, k, k, P.b2g.data_ptr() + 4 * P.cut[i], 2.0 ** eB, 2.0 ** eB * LOG2E, s_b,
                                dst.data_ptr(), 32 * nb, _st()) == 0
        keep.append(dst)
        segs[i] = _lib.Segment(P.cut[i], P.cut[i + 1], k, P.t_off[i], dst.data_ptr(), 32 * nb)
        ts[i], ds[i], s8[i] = 2.0 ** eT_i, 2.0 ** -(eT_i + eB), s_b
    return segs, ts, ds, s8, keep


# ---------------------------------------------------------------------------------------------------------------- one launch
def _guarded_part(bound):
    ld = bound + GUARD_ROWS
    part = torch.empty((MAXP + GUARD_SLICES, ld, 2), dtype=torch.float32, device="cuda")
    part.view(torch.int32).fill_(int(NAN_BITS))
    return part, ld


def _guarded_lse(G):
    return torch.full((G,), LSE_SENTINEL, dtype=torch.float64, device="cuda")


def _nd(n):
    return None if n is None else torch.as_tensor(np.array([n], dtype=np.int32)).cuda()


# Peaked rows: the forms that miss the 2e-6 bar there, with the largest error measured on the MI355X as a fraction of max(1, |lse|).  The
# top word's logit is a 22-25 nat dot product, and its int8 / FP6 cross terms are quantised against the row's and the segment's largest
# values: a property of the row format, not of a kernel (the split and f32 forms of the same rows meet their bars).  Such rows are what the
# loader keeps off those formats: test_gpu_mixed_logits.py::GATES, checked by test_peaked_misses_are_formats_the_loader_refuses.  The bar
# there is the measured figure with a margin of PEAKED_MARGIN -- a dropped tile or a lost maximum is off by nats.
PEAKED_MISS = {"MX_KERNEL_DSOFTMAX": 2.92e-6, "MX_KERNEL_GENERIC": 4.06e-6, "MX_KERNEL_GENERIC_XB": 2.98e-6, "MXW_KERNEL_DSOFTMAX": 2.92e-6,
               "MX6_KERNEL_DSOFTMAX": 8.73e-6, "MX6_KERNEL_DSOFTMAX_FR": 8.72e-6, "MX6_KERNEL_GENERIC": 1.2e-5, "MX6_KERNEL_GENERIC_XB": 6.36e-6,
               "MX6_KERNEL_TIED": 3.85e-6, "MX6_KERNEL_TIED_FR": 3.85e-6, "MX6W_KERNEL_DSOFTMAX": 8.73e-6, "MX6W_KERNEL_DSOFTMAX_FR": 8.72e-6,
               "MX6W_KERNEL_TIED": 3.85e-6, "MX6W_KERNEL_TIED_FR": 3.85e-6,
               "hybrid-tail-split": 2.54e-6, "hybrid-head-256": 2.92e-6, "hybrid-first-split": 2.92e-6, "hybrid-heads": 2.92e-6}
# (met on the same rows, so held to 2e-6: MX_KERNEL_TIED 1.87e-6, MXW_KERNEL_TIED(_FR) 1.87e-6, MXW_KERNEL_K512(_FR) 1.78e-6; the split
#  and f32 stationary forms 4.7e-7)
PEAKED_MARGIN = 1.5
LAST = {}                                     # what the last launch left: slice count, the sampled rows' lse (forms_agree, np sweep)


def _check(P, part, n_slices, lse, n, bar, what, fixed_ref_overflow=False, peaked_key=None):
    """the assertions every case makes (see the module's docstring); returns the largest error against f64.  peaked_key: the form's key
    in PEAKED_MISS"""
    torch.cuda.synchronize()
    LAST.clear()
    LAST["ns"] = n_slices
    live = _live(P.bound, n)
    bits = part.cpu().numpy().view(np.uint32)
    assert 1 <= n_slices <= MAXP, (what, n_slices)
    # nothing outside [0, live) x [0, n_slices) written: guard slices, guard rows, and the rows past the count of the written slices
    outside = np.ones(bits.shape[:2], dtype=bool)
    outside[:n_slices, :live] = False
    bad = np.argwhere(outside & (bits != NAN_BITS).any(axis=2))
    assert len(bad) == 0, (what, "cells written outside the live rows (slice, row):", bad[:8].tolist(), len(bad))
    got = lse.cpu().numpy()
    listed = np.zeros(P.G, dtype=bool)
    listed[P.rows[:live]] = True
    assert (got[~listed] == LSE_SENTINEL).all(), (what, "lse of rows not stepped changed", np.argwhere(got[~listed] != LSE_SENTINEL)[:8])
    s = P.sample[P.sample < live]
    if len(s) == 0:
        return 0.0
    g = got[P.rows[s]]
    LAST["lse"] = g.copy()
    ref = P.ref[P.sample < live]
    if fixed_ref_overflow:
        assert not np.isfinite(g).any(), (what, "a fixed-reference form returned a finite lse past the f32 range", g[np.isfinite(g)][:4])
        return 0.0
    err = np.abs(g - ref)
    assert np.isfinite(g).all(), (what, "non-finite lse", np.argwhere(~np.isfinite(g))[:8])
    lim = bar(ref)
    LAST["rel"] = float(err.max()) / max(1.0, float(np.abs(ref).max()))
    if P.regime == "peaked" and peaked_key in PEAKED_MISS:
        lim = PEAKED_MARGIN * PEAKED_MISS[peaked_key] * max(1.0, float(np.abs(ref).max()))
    worst = int(np.argmax(err - lim))
    assert (err <= lim).all(), (what, "lse vs f64: row", int(s[worst]), float(g[worst]), float(ref[worst]), float(err[worst]))
    return float(err.max())


def _mixed_bar(ref):
    return 2e-6 * max(1.0, float(np.abs(ref).max()))


def _record(case_id, kind, form, err):
    if OUT:
        with open(os.path.join(OUT, "cases.jsonl"), "a") as f:
            f.write(json.dumps({"id": case_id, "kind": kind, "form": form, "err": err, "rel": LAST.get("rel")}) + "\n")


def _save_ident(key, arr):
    """the children of the forced-form tests leave the results of the fixed cases the forms are compared on (check_forced_child)"""
    if OUT and key in IDENT:
        np.save(os.path.join(OUT, "ident-%s.npy" % key), arr)


def run_mixed(L, P, layout, fmt, fr, n):
    segs, ts, ds, s8, keep = _mixed_rows(L, P, fmt)
    nseg = len(P.widths)
    b2l = (P.b2g * LOG2E).contiguous()
    bias2 = b2l.data_ptr() if P.widths[0] % 32 == 0 else None
    form = L.jlm_vocab_lse_mixed_form(segs, ds, s8, int(bias2 is not None), nseg, fr)
    assert form == FK.jlm_vocab_lse_mixed_form(segs, ds, s8, int(bias2 is not None), nseg, fr)
    want = expected_mixed_form(layout, fmt, fr, _env())
    assert MX_FORMS[form] == want, (layout, fmt, fr, MX_FORMS[form], want)
    ld_tm = L.jlm_mixed_t_stride(segs, nseg)
    Tm = torch.zeros(((P.bound + 255) // 256 * 256, ld_tm), dtype=torch.float32, device="cuda")
    nd = _nd(n)
    ndp = nd.data_ptr() if nd is not None else None
    assert _pack_t(L, fmt)(segs, ts, nseg, P.Tg.data_ptr(), P.ldt, P.rows_g.data_ptr(), P.bound, ndp, Tm.data_ptr(), ld_tm, _st()) == 0
    part, ld = _guarded_part(P.bound)
    lse = _guarded_lse(P.G)
    entry = L.jlm_vocab_lse_mixed_fr if fr else L.jlm_vocab_lse_mixed
    ns = entry(segs, ds, s8, bias2, nseg, Tm.data_ptr(), ld_tm, part.data_ptr(), ld, MAXP, P.bound, ndp, _st())
    assert ns >= nseg, ns
    assert L.jlm_lse_combine(part.data_ptr(), ld, ns, P.rows_g.data_ptr(), lse.data_ptr(), P.bound, ndp, _st()) == 0
    overflow = P.regime == "shift_beyond" and want in FIXED_REF_FORMS
    err = _check(P, part, ns, lse, n, _mixed_bar, (layout, fmt, fr, P.bound, n, P.regime, want), overflow, MX_FORMS[form])
    return MX_FORMS[form], err


def run_split(L, P, n):
    nseg = len(P.widths)
    plain = (_lib.Segment * nseg)(*[_lib.Segment(P.cut[i], P.cut[i + 1], k, P.t_off[i], P.Bg[i].data_ptr(), k) for i, k in enumerate(P.widths)])
    sp, ts, ds, bc, keep = _split_segments(L, plain, None, nseg, [6] * nseg, P.b2g)
    waves = L.jlm_vocab_lse_split_form()
    assert waves == FK.jlm_vocab_lse_split_form() == (4 if _env()["waves"] == 4 else 8)
    nd = _nd(n)
    ndp = nd.data_ptr() if nd is not None else None
    errs = {}
    for name in ("f32", "split"):
        part, ld = _guarded_part(P.bound)
        lse = _guarded_lse(P.G)
        if name == "f32":
            ns = L.jlm_vocab_lse_stationary(plain, nseg, P.b2g.data_ptr(), P.Tg.data_ptr(), P.ldt, P.rows_g.data_ptr(), part.data_ptr(), ld,
                                            MAXP, P.bound, ndp, _st())
        else:
            ns = L.jlm_vocab_lse_split(sp, ts, ds, bc, nseg, P.b2g.data_ptr(), P.Tg.data_ptr(), P.ldt, P.rows_g.data_ptr(), part.data_ptr(),
                                       ld, MAXP, P.bound, ndp, _st())
        assert ns >= nseg, (name, ns)
        assert L.jlm_lse_combine(part.data_ptr(), ld, ns, P.rows_g.data_ptr(), lse.data_ptr(), P.bound, ndp, _st()) == 0
        bar = _mixed_bar if name == "f32" else (lambda ref: 2e-5)
        errs[name] = _check(P, part, ns, lse, n, bar, (name, P.widths, P.bound, n, P.regime))
    assert errs["split"] < 4 * errs["f32"] + 2e-6, errs
    return waves, errs


def run_hybrid(L, P, form, n):
    mixed_set, heads = HYBRID[form]
    nseg = 3
    mx, ts, ds, s8, keep = _mixed_rows(L, P, "int8")
    plain = (_lib.Segment * nseg)(*[_lib.Segment(P.cut[i], P.cut[i + 1], k, P.t_off[i], P.Bg[i].data_ptr(), k) for i, k in enumerate(P.widths)])
    sp, sts, sds, bc, keep2 = _split_segments(L, plain, None, nseg, [6] * nseg, P.b2g)
    for i in range(nseg):
        sts[i], sds[i] = 2.0 ** 10, 2.0 ** -(10 + 6)
    mixed = (_lib.Segment * nseg)()
    for i in mixed_set:
        mixed[i] = mx[i]
    nm = len(mixed_set)
    only = (_lib.Segment * nm)(*[mx[i] for i in mixed_set])
    ld_tm = L.jlm_mixed_t_stride(only, nm)
    Tm = torch.zeros(((P.bound + 255) // 256 * 256, ld_tm), dtype=torch.float32, device="cuda")
    nd = _nd(n)
    ndp = nd.data_ptr() if nd is not None else None
    assert L.jlm_pack_t_mixed(only, (ctypes.c_float * nm)(*[ts[i] for i in mixed_set]), nm, P.Tg.data_ptr(), P.ldt, P.rows_g.data_ptr(),
                              P.bound, ndp, Tm.data_ptr(), ld_tm, _st()) == 0
    part, ld = _guarded_part(P.bound)
    lse = _guarded_lse(P.G)
    hs = (ctypes.c_int * nseg)(*heads) if heads else None
    ns = L.jlm_vocab_lse_hybrid(sp, sts, sds, bc, mixed, ds, s8, hs, nseg, P.b2g.data_ptr(), P.Tg.data_ptr(), P.ldt, Tm.data_ptr(), ld_tm,
                                P.rows_g.data_ptr(), part.data_ptr(), ld, MAXP, P.bound, ndp, _st())
    assert ns >= nseg + (sum(1 for c in heads if c) if heads else 0), ns
    assert L.jlm_lse_combine(part.data_ptr(), ld, ns, P.rows_g.data_ptr(), lse.data_ptr(), P.bound, ndp, _st()) == 0
    return _check(P, part, ns, lse, n, _mixed_bar, ("hybrid", form, P.bound, n, P.regime), peaked_key="hybrid-" + form)


# ---------------------------------------------------------------------------------------------------------------- cases
def _mixed_cases():
    out = []
    for layout in MIXED_LAYOUTS:
        for fmt in ("int8", "mx6"):
            if fmt == "mx6" and layout == "k512":
                continue                                     # (refused: tests/test_lse_dispatch_cpu.py)
            for fr in (0, 1):
                for bound in BOUNDS:
                    out += [(layout, fmt, fr, bound, n, "gauss") for n in _counts(bound)]
                    out += [(layout, fmt, fr, bound, n, regime) for regime in ("peaked", "shift39", "shift_beyond")
                            for n in (bound - 1, None) if bound in (300, 2560)]
    return out


def _mixed_id(c):
    layout, fmt, fr, bound, n, regime = c
    return "%s-%s-%s-B%d-n%s-%s" % (layout, fmt, "fr" if fr else "max", bound, "NULL" if n is None else n, regime)


MIXED_CASES = _mixed_cases()


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.lib()


@pytest.mark.parametrize("case", MIXED_CASES, ids=_mixed_id)
def test_mixed_form(L, case):
    layout, fmt, fr, bound, n, regime = case
    P = problem(MIXED_LAYOUTS[layout], bound, regime)
    form, err = run_mixed(L, P, layout, fmt, fr, n)
    _record("mixed-" + _mixed_id(case), "mixed", form, err)
    _save_ident("mixed-" + _mixed_id(case), LAST.get("lse"))


BIG_MIXED = [("dsoftmax", "int8", 0), ("dsoftmax", "mx6", 0), ("dsoftmax", "mx6", 1), ("tied", "int8", 0), ("tied", "int8", 1),
             ("tied", "mx6", 0), ("tied", "mx6", 1), ("k512", "int8", 0), ("k512", "int8", 1)]


@pytest.mark.parametrize("n", [BIG - 1, None], ids=["n20479", "nNULL"])
@pytest.mark.parametrize("layout,fmt,fr", BIG_MIXED, ids=["-".join(map(str, c)) for c in BIG_MIXED])
def test_mixed_form_20480_rows(L, layout, fmt, fr, n):
    P = problem(MIXED_LAYOUTS[layout], BIG, "gauss", vocab=50000)
    form, err = run_mixed(L, P, layout, fmt, fr, n)
    _record("mixed-big-%s-%s-%d-%s" % (layout, fmt, fr, n), "mixed", form, err)


def _split_cases():
    out = []
    for layout in SPLIT_LAYOUTS:
        for bound in BOUNDS:
            out += [(layout, bound, n, "gauss") for n in _counts(bound)]
            out += [(layout, bound, n, regime) for regime in ("peaked", "shift_beyond") for n in (bound - 1, None) if bound in (300, 2560)]
    return out + [("dsoftmax", BIG, n, "gauss") for n in (BIG - 1, None)]


@pytest.mark.parametrize("case", _split_cases(), ids=lambda c: "%s-B%d-n%s-%s" % (c[0], c[1], "NULL" if c[2] is None else c[2], c[3]))
def test_split_form(L, case):
    layout, bound, n, regime = case
    P = problem(SPLIT_LAYOUTS[layout], bound, regime, vocab=50000 if bound == BIG else V)
    waves, errs = run_split(L, P, n)
    _record("split-%s-B%d-n%s-%s" % case, "split", waves, errs["split"])
    _save_ident("split-%s-B%d-n%s-%s" % case, LAST.get("lse"))
    _record("stationary-%s-B%d-n%s-%s" % case, "stationary", 0, errs["f32"])


def _hybrid_cases():
    out = []
    for form in HYBRID:
        for bound in BOUNDS:
            out += [(form, bound, n, "gauss") for n in _counts(bound)]
            out += [(form, bound, n, "peaked") for n in (bound - 1, None) if bound in (300, 2560)]
    return out + [("tail-split", BIG, n, "gauss") for n in (BIG - 1, None)]


@pytest.mark.parametrize("case", _hybrid_cases(), ids=lambda c: "%s-B%d-n%s-%s" % (c[0], c[1], "NULL" if c[2] is None else c[2], c[3]))
def test_hybrid_form(L, case):
    form, bound, n, regime = case
    P = problem([200, 100, 52], bound, regime, vocab=50000 if bound == BIG else V)
    err = run_hybrid(L, P, form, n)
    _record("hybrid-%s-B%d-n%s-%s" % case, "hybrid", 0, err)


@pytest.mark.parametrize("np_force", ["1", "7", "24", "cap"])
@pytest.mark.parametrize("launch", ["split", "mixed-dsoftmax-int8", "mixed-dsoftmax-mx6", "mixed-tied-int8"])
def test_lse_np_sweep(L, monkeypatch, launch, np_force):
    """JLM_LSE_NP (read on every call) moves the column cuts across the segment boundaries; peaked rows put the top word on both sides of
    every 32-word edge of a segment, so of every cut"""
    widths = [256] if "tied" in launch else [200, 100, 52]
    cap = MAXP - (len(widths) - 1)
    f = cap if np_force == "cap" else int(np_force)
    monkeypatch.setenv("JLM_LSE_NP", str(f))
    for regime in ("gauss", "peaked"):
        P = problem(widths, 2560, regime)
        if launch == "split":
            run_split(L, P, 2559)
            tiles = [(P.cut[i + 1] - P.cut[i] + 127) // 128 for i in range(len(widths))]
        else:
            _, layout, fmt = launch.split("-")
            run_mixed(L, P, layout, fmt, 0, 2559)
            tiles = [(P.cut[i + 1] - P.cut[i] + _mx_tile(k) - 1) // _mx_tile(k) for i, k in enumerate(widths)]
        # the forced column count took effect: at most min(f, tiles) columns of whole tiles -- as few as ceil(tiles / ceil(tiles / f)) where
        # equal-cost columns cannot make f (32 tiles into 24 columns: 16 of two tiles) -- one slice per column plus one per segment
        # boundary a column straddles
        t = sum(tiles)
        assert -(-t // -(-t // f)) <= LAST["ns"] <= min(f, t) + len(widths) - 1, (launch, f, tiles, LAST["ns"])


def _mx_tile(k):
    """words per vocabulary tile of a mixed segment: 32 x mx_blocks_per_tile(blocks of 32 k) (csrc/jlm_mixed_body.h)"""
    nb = k // 32 if k % 32 == 0 else (k + 2 + 31) // 32
    return 32 * (1 if nb >= 9 else 2 if nb >= 5 else 4 if nb >= 3 else 8)


def test_peaked_misses_are_formats_the_loader_refuses():
    """every form in PEAKED_MISS runs int8 or mx6 cross terms, and the loader keeps models whose logits reach +-20 off those planes
    wherever they carry the peaked words: test_gpu_mixed_logits.py::GATES -- peaked20-vtable keeps int8 rows on its later segments only
    (the first, which carries the mass, on split rows; mx6 refused), peaked20-tied keeps no mixed rows at all"""
    from tests.test_gpu_mixed_logits import GATES
    assert ("peaked20-vtable", "first-split", "int8") in GATES
    assert ("peaked20-tied", False, None) in GATES
    for key in PEAKED_MISS:
        assert key.startswith(("MX_", "MXW_", "MX6_", "MX6W_", "hybrid-")), key


# ---------------------------------------------------------------------------------------------------------------- T projection
T_SHAPES = [(700, 352, 512), (2560, 256, 512), (2560, 352, 256), (10240, 256, 512), (20480, 256, 512), (4096, 2048, 512)]


def _t_counts(M):
    c = [n for n in (0, 1, 63, 64, 65, 127, 128, 129) if n < M]
    return c + [M - 1, M, M + 7, None]


def _t_cases():
    return [(M, N, K, n, gather) for M, N, K in T_SHAPES for n in _t_counts(M) for gather in (True, False)
            if gather or n in (None, M - 1, 0)]


@pytest.mark.parametrize("case", _t_cases(), ids=lambda c: "M%d-N%d-K%d-n%s-%s" % (c[0], c[1], c[2], "NULL" if c[3] is None else c[3],
                                                                                  "rows" if c[4] else "plain"))
def test_t_projection_form(L, case):
    """jlm_gemm_nt_split (the decode's T projection) on every path of its dispatch, gathered / scattered rows and device counts, against
    float64 of the f32 operands; C rows not in rows[:count] stay bit for bit"""
    M, N, K, n, gather = case
    env = _env()
    form = L.jlm_gemm_nt_split_form(M, N)
    assert form == FK.jlm_gemm_nt_split_form(M, N)
    tiles64 = ((M + 63) // 64) * ((N + 63) // 64)
    if tiles64 <= 256 and env["stages"] == 3:
        assert T_FORMS[form] == ("SPLIT3_LINEAR" if env["xcd"] == 0 else "SPLIT3_XCD")
    else:
        assert T_FORMS[form] == ("CFG64" if ((M + 127) // 128) * ((N + 127) // 128) < 512 else "CFG128")
    rng = np.random.default_rng(M * 7 + N + K)
    GA = M + 9 if gather else M
    A = rng.standard_normal((GA, K)).astype(np.float32)
    B = (rng.standard_normal((N, K)) * 0.1).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    ldc = N + 4
    Ag, Bg, biasg = (torch.as_tensor(x).cuda() for x in (A, B, bias))
    As, Bs = _pack(L, Ag, K, 2.0 ** 10), _pack(L, Bg, K, 2.0 ** 12)
    C = torch.empty((GA, ldc), dtype=torch.float32, device="cuda")
    C.view(torch.int32).fill_(int(NAN_BITS))
    rows = (rng.permutation(GA)[:M].astype(np.int32)) if gather else np.arange(M, dtype=np.int32)
    rows_g = torch.as_tensor(rows).cuda() if gather else None
    rp = rows_g.data_ptr() if gather else None
    nd = _nd(n) if (gather or n is not None) else None
    ndp = nd.data_ptr() if nd is not None else None
    assert L.jlm_gemm_nt_split(As.data_ptr(), K, rp, Bs.data_ptr(), K, None, C.data_ptr(), ldc, rp, biasg.data_ptr(), 2.0 ** -22, M, N, K,
                               ndp, _st()) == 0
    torch.cuda.synchronize()
    live = M if n is None else min(n, M)
    got = C.cpu().numpy()
    bits = got.view(np.uint32)
    sel = rows[:live]
    ref = A[sel].astype(np.float64) @ B.astype(np.float64).T + bias.astype(np.float64)
    np.testing.assert_allclose(got[sel, :N], ref, rtol=2e-5, atol=1e-5)
    untouched = np.ones(GA, dtype=bool)
    untouched[sel] = False
    assert (bits[untouched] == NAN_BITS).all(), "C rows outside rows[:count] written"
    assert (bits[sel, N:] == NAN_BITS).all(), "C columns past N written"
    _record("t-M%d-N%d-K%d-n%s-%s" % case, "t", form, 0.0)
    LAST["lse"] = got[sel, :N].copy()
    _save_ident("t-M%d-N%d-K%d-n%s-%s" % case, LAST["lse"])


# ---------------------------------------------------------------------------------------------------------------- forced forms
# the fixed cases the forms of one launch are compared on, per setting (check_forced_child): the child's result against the default
# form's, computed in the parent
_B = "B2560-n2559-gauss"
_I8 = ["mixed-%s-int8-%s-%s" % (lay, e, _B) for lay in ("dsoftmax", "tied") for e in ("max", "fr")]
_M6 = ["mixed-%s-mx6-%s-%s" % (lay, e, _B) for lay in ("dsoftmax", "tied") for e in ("max", "fr")]
IDENT_OF = {"JLM_MX_WIDE=1": _I8, "JLM_MX_WIDE=0": _I8, "JLM_MX6_WIDE=1": _M6, "JLM_MX6_WIDE=0": _M6,
            "JLM_LSE_WAVES=4": ["split-dsoftmax-" + _B],
            "JLM_T_STAGES=4": ["t-M2560-N256-K512-n2559-True"],
            "JLM_T_XCD=0": ["t-M2560-N256-K512-n2559-True"]}
IDENT = {k for v in IDENT_OF.values() for k in v}
# measured on the MI355X: the cases on which the forced form's results are bit-identical to the default form's.  The others differ in the
# last bits (the wide and eight-wave kernels fold in another order: 4e-8 .. 6.5e-8 on an lse of ~7.7) and are held to the case's bar.
IDENTICAL = {("JLM_MX_WIDE=0", "mixed-dsoftmax-int8-max-" + _B), ("JLM_MX_WIDE=0", "mixed-dsoftmax-int8-fr-" + _B),
             ("JLM_MX_WIDE=1", "mixed-tied-int8-max-" + _B), ("JLM_MX_WIDE=1", "mixed-tied-int8-fr-" + _B),
             ("JLM_MX6_WIDE=0", "mixed-tied-mx6-fr-" + _B), ("JLM_MX6_WIDE=1", "mixed-dsoftmax-mx6-fr-" + _B),
             ("JLM_LSE_WAVES=4", "split-dsoftmax-" + _B), ("JLM_T_STAGES=4", "t-M2560-N256-K512-n2559-True"),
             ("JLM_T_XCD=0", "t-M2560-N256-K512-n2559-True")}


def _rerun(L, key):
    """run one fixed case in this process (the default forms) -> its result"""
    kind, rest = key.split("-", 1)
    if kind == "mixed":
        case = [c for c in MIXED_CASES if "mixed-" + _mixed_id(c) == key][0]
        test_mixed_form(L, case)
    elif kind == "split":
        case = [c for c in _split_cases() if "split-%s-B%d-n%s-%s" % c == key][0]
        test_split_form(L, case)
    else:
        case = [c for c in _t_cases() if "t-M%d-N%d-K%d-n%s-%s" % c == key][0]
        test_t_projection_form(L, case)
    return LAST["lse"]


# setting -> (pytest -k of this module, -k of test_gpu_kernels.py, the case records it serves, the form each of them must report)
FORCED = {
    "JLM_MX_WIDE=1": ("test_mixed_form and int8 or test_lse_np_sweep and int8", "test_vocab_lse_mixed",
                      lambda c: c["kind"] == "mixed" and "dsoftmax-int8" in c["id"], lambda c: "MXW_KERNEL_DSOFTMAX"),
    "JLM_MX_WIDE=0": ("test_mixed_form and int8 or test_lse_np_sweep and int8", "test_vocab_lse_mixed",
                      lambda c: c["kind"] == "mixed" and "tied-int8" in c["id"], lambda c: "MX_KERNEL_TIED"),
    "JLM_MX6_WIDE=1": ("test_mixed_form and mx6 or test_lse_np_sweep and mx6", "test_vocab_lse_mixed",
                       lambda c: c["kind"] == "mixed" and "dsoftmax-mx6" in c["id"],
                       lambda c: "MX6W_KERNEL_DSOFTMAX_FR" if "-fr-" in c["id"] or "-mx6-1-" in c["id"] else "MX6W_KERNEL_DSOFTMAX"),
    "JLM_MX6_WIDE=0": ("test_mixed_form and mx6 or test_lse_np_sweep and mx6", "test_vocab_lse_mixed",
                       lambda c: c["kind"] == "mixed" and "tied-mx6" in c["id"],
                       lambda c: "MX6_KERNEL_TIED_FR" if "-fr-" in c["id"] or "-mx6-1-" in c["id"] else "MX6_KERNEL_TIED"),
    "JLM_LSE_WAVES=4": ("test_split_form or test_lse_np_sweep and split", "test_vocab_lse_split",
                        lambda c: c["kind"] == "split", lambda c: 4),
    "JLM_T_STAGES=4": ("test_t_projection_form", "test_gemm_nt_split",
                       lambda c: c["kind"] == "t", lambda c: T_FORMS.index("CFG64") if "-N2048-" not in c["id"] else T_FORMS.index("CFG128")),
    "JLM_T_XCD=0": ("test_t_projection_form", "test_gemm_nt_split",
                    lambda c: c["kind"] == "t" and ("M700-" in c["id"] or "M2560-" in c["id"]), lambda c: T_FORMS.index("SPLIT3_LINEAR")),
}


def _expected_ids(label):
    """the records a child of this setting must leave: every case of this module its -k selects that the forced form serves"""
    serves = FORCED[label][2]
    ids = ["mixed-" + _mixed_id(c) for c in MIXED_CASES]
    ids += ["mixed-big-%s-%s-%d-%s" % (lay, fmt, fr, n) for lay, fmt, fr in BIG_MIXED for n in (BIG - 1, None)]
    ids += ["split-%s-B%d-n%s-%s" % c for c in _split_cases()]
    ids += ["t-M%d-N%d-K%d-n%s-%s" % c for c in _t_cases()]
    kind = lambda i: i.split("-")[0]
    return [i for i in ids if serves({"id": i, "kind": kind(i)})]


def check_forced_child(label, tmp_path):
    """test_gpu_kernels.py::test_vocab_lse_forced_forms: the child of one forced setting passed, ran every case of this module the forced
    form serves (and the kernel tests of that launcher), and each of those cases reported the forced form"""
    import subprocess
    import sys
    k_here, k_kernels, serves, want = FORCED[label]
    name, value = label.split("=")
    out = str(tmp_path)
    env = dict(os.environ, JLM_LSE_FORMS_OUT=out)
    env[name] = value
    here = os.path.abspath(__file__)
    kern = os.path.join(os.path.dirname(here), "test_gpu_kernels.py")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", here, "-k", k_here]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-1000:]
    r2 = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", kern, "-k",
                         k_kernels + " and not forced"], env=env, capture_output=True, text=True, timeout=900)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-2000:]
    assert " passed" in r2.stdout and "failed" not in r2.stdout, r2.stdout[-1000:]
    with open(os.path.join(out, "cases.jsonl")) as f:
        ran = {}
        for line in f:
            c = json.loads(line)
            ran[c["id"]] = c
    expected = _expected_ids(label)
    assert expected, label
    missing = [i for i in expected if i not in ran]
    assert not missing, (label, len(missing), missing[:8])
    served = [c for c in ran.values() if serves(c)]
    wrong = [(c["id"], c["form"], want(c)) for c in served if c["form"] != want(c)]
    assert not wrong, (label, len(wrong), wrong[:8])
    print(label, "cases served:", len(served), "of", len(ran))
    # the forced form against the default form on the same inputs
    L = _lib.lib()
    for key in IDENT_OF[label]:
        got = np.load(os.path.join(out, "ident-%s.npy" % key))
        ref = _rerun(L, key)
        assert got.shape == ref.shape, (label, key)
        diff = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
        print(label, key, "bit-identical" if np.array_equal(got, ref) else "largest difference %.3g" % diff)
        if (label, key) in IDENTICAL:
            np.testing.assert_array_equal(got, ref, err_msg="%s %s" % (label, key))
