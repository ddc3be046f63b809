"""GPU: score_fold_kernel (csrc/jlm_score.hip) called directly through jlm_score_fold, against the float64 restatement of its contract
(tests/fake_hip.py FakeLib.jlm_score_fold) on the same f32 operands.

What a case varies, each against the kernel's own thresholds:

* the slice count against the four-deep unrolled fold (p + 24 < n_parts) and the 8-lane split: 1, 7, 8, 9, 24, 25, 31, 32, 33, 57, 96.
  Slice maxima are spread over +-30 nats (the rescaling matters), a tenth of the slices are (-big, 0) as an empty tile leaves them;
  `part` has guard rows and guard slices filled with NaN (as tests/test_gpu_lse_forms.py fills them);
* the 32 rows of a workgroup against the row bound and the device count: bounds 1, 31, 32, 33, 100; n_dev NULL, 0, 1, bound - 1, bound,
  bound + 7; rows past the count keep their sentinels in nll_seq and nll_tok;
* the target's logit: layouts [4] (K4 = 1: seven lanes idle), [8, 36], [200, 100, 52], [256] (all 64 chunks in registers, no tail),
  [260] (one lane runs the tail loop once) and [512]; ldt has slack; targets on the first and last word of every segment and uniform;
* both SELF_NORM instantiations, nll_tok NULL or not, flags NULL or not, the += into nll_seq over two calls;
* a target of -1 and of v_end of the last segment (bit 2, NaN, the other rows right; the kernel reads nothing of B, T or b2 for such a
  row: brow stays NULL and every load behind it is under `if (brow)`), a non-finite slice sum (bit 1).

Bars, from the project's other tests and not from this kernel: the log-normaliser 2e-6 x max(1, |ref|) (the normaliser bar of
tests/test_gpu_lse_forms.py), the logit rtol = atol = 2e-5 at the operand scale of test_gpu_kernels.py::test_edge_logits (weights
0.3 N(0, 1), T and b2 N(0, 1)); nll their sum.  Each part is also measured alone: zero weights and biases leave the fold, self_norm
leaves the logit (the measured maxima are in DESIGN.md beside score_fold_kernel).

The header comment's two claims are checked once each, bit for bit: the logit against jlm_edge_logits on the same (row, word), the
fold against jlm_beam_step's fused combine on the same slices."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                      # noqa: E402
from tests.fake_hip import NEG, FakeLib                                       # noqa: E402
from tests.test_gpu_kernels import _beam_problem, _segments, _st              # noqa: E402

pytestmark = pytest.mark.gpu

FK = FakeLib()
V = 301
N_PARTS = (1, 7, 8, 9, 24, 25, 31, 32, 33, 57, 96)
BOUNDS = (1, 31, 32, 33, 100)
LAYOUTS = {"k4": [4], "k8_36": [8, 36], "dsoftmax": [200, 100, 52], "k256": [256], "k260": [260], "k512": [512]}
GUARD_SLICES, GUARD_ROWS = 3, 11
SEQ0, TOK0 = 1000.5, -777.25
MEASURED = {"fold": 0.0, "logit": 0.0}       # the largest error of each part alone, as a fraction of its bar's scale (printed per test)


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.lib()


class Problem:
    """operands of one (widths, bound, n_parts): on the host for the restatement, on the device for the kernel"""

    def __init__(self, widths, bound, n_parts, zero_logit=False, seed=0):
        rng = np.random.default_rng(zlib.crc32(repr((widths, bound, n_parts, zero_logit, seed)).encode()))
        self.widths, self.bound, self.n_parts = list(widths), bound, n_parts
        self.segs_c, self.segs_g, self.keep, self.ldt = _segments(rng, V, widths, ldt_extra=8)
        self.nseg = len(widths)
        self.rows_alloc = bound + GUARD_ROWS
        self.T = rng.standard_normal((self.rows_alloc, self.ldt)).astype(np.float32)
        self.b2 = rng.standard_normal(V).astype(np.float32)
        if zero_logit:
            for t in self.keep:
                t.zero_()
            self.b2[:] = 0.0
        self.ld_part = self.rows_alloc
        part = np.full((n_parts + GUARD_SLICES, self.ld_part, 2), np.nan, dtype=np.float32)
        part[:n_parts, :bound, 0] = rng.uniform(-30.0, 30.0, size=(n_parts, bound))
        part[:n_parts, :bound, 1] = rng.uniform(1.0, 128.0, size=(n_parts, bound))
        empty = rng.random((n_parts, bound)) < 0.1
        empty[0] = False                                          # never every slice of a row
        part[:n_parts, :bound][empty] = (NEG, 0.0)
        self.part = part
        edges = [w for i in range(self.nseg) for w in (self.segs_c[i].v_start, self.segs_c[i].v_end - 1)]
        tgt = rng.integers(0, V, size=self.rows_alloc)
        tgt[:min(len(edges), bound)] = edges[:bound]
        self.target = tgt.astype(np.int32)

    def segs(self, cuda):
        return self.segs_g if cuda else self.segs_c


def run(lib, P, cuda, n, self_norm, tok=True, flags=True, calls=1, part=None, target=None):
    """`calls` consecutive jlm_score_fold launches over the same operands -> nll_seq, nll_tok (None), flags (None), all rows allocated"""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda() if cuda else torch.as_tensor(np.ascontiguousarray(a)).clone()
    T, b2, pt = t(P.T), t(P.b2), t(P.part if part is None else part)
    tg = t(P.target if target is None else target)
    seq = t(SEQ0 + np.arange(P.rows_alloc, dtype=np.float64))
    tk = t(np.full(P.rows_alloc, TOK0)) if tok else None
    fl = t(np.zeros(1, dtype=np.int32)) if flags else None
    nd = None if n is None else t(np.array([n], dtype=np.int32))
    for _ in range(calls):
        rc = lib.jlm_score_fold(P.segs(cuda), P.nseg, b2.data_ptr(), T.data_ptr(), P.ldt, pt.data_ptr(), P.ld_part, P.n_parts, self_norm,
                                tg.data_ptr(), nd.data_ptr() if nd is not None else None, P.bound, seq.data_ptr(),
                                tk.data_ptr() if tok else None, fl.data_ptr() if flags else None, _st() if cuda else 0)
        assert rc == 0, rc
    if cuda:
        torch.cuda.synchronize()
    return dict(seq=seq.cpu().numpy(), tok=tk.cpu().numpy() if tok else None, flags=int(fl.cpu().numpy()[0]) if flags else None)


def parts_of(P, n):
    """the float64 log-normaliser and logit of rows < n, each alone (the restatement run twice)"""
    y = -(run(FK, P, False, n, 1)["tok"])
    lse = run(FK, P, False, n, 0)["tok"] + y
    return lse, y


def bar(P, n, self_norm, lse, y):
    """per live row: the normaliser bar of test_gpu_lse_forms.py plus the logit bar of test_edge_logits"""
    b = 2e-5 + 2e-5 * np.abs(y[:n])
    if not self_norm:
        b = b + 2e-6 * np.maximum(1.0, np.abs(lse[:n]))
    return b


def check(L, P, n, self_norm, tok=True, flags=True, calls=1, skip=(), **kw):
    """kernel against restatement: live rows within the bar (`skip`: rows judged by the caller), every other row's sentinels untouched"""
    live = P.bound if n is None else min(n, P.bound)
    want = run(FK, P, False, n, self_norm, tok, flags, calls, **kw)
    got = run(L, P, True, n, self_norm, tok, flags, calls, **kw)
    lse, y = parts_of(P, n) if live else (np.zeros(0), np.zeros(0))
    lim = bar(P, live, self_norm, lse, y)
    keep = np.ones(live, dtype=bool)
    keep[[r for r in skip if r < live]] = False
    sentinel = SEQ0 + np.arange(P.rows_alloc, dtype=np.float64)
    np.testing.assert_array_equal(got["seq"][live:], sentinel[live:], err_msg="nll_seq past the count")
    with np.errstate(invalid="ignore"):                       # (a skipped row may hold inf on both sides)
        err = np.abs(got["seq"][:live] - want["seq"][:live])[keep]
    assert np.isfinite(got["seq"][:live][keep]).all()
    assert (err <= calls * lim[keep]).all(), ("nll_seq", float(err.max()), int(np.argmax(err - calls * lim[keep])))
    if tok:
        np.testing.assert_array_equal(got["tok"][live:], np.full(P.rows_alloc - live, TOK0), err_msg="nll_tok past the count")
        with np.errstate(invalid="ignore"):
            e = np.abs(got["tok"][:live] - want["tok"][:live])[keep]
        assert (e <= lim[keep]).all(), ("nll_tok", float(e.max()), int(np.argmax(e - lim[keep])))
        # nll_seq is the sentinel plus the step's nll, `calls` times, in f64
        acc = sentinel[:live].copy()
        for _ in range(calls):
            acc = acc + got["tok"][:live]
        np.testing.assert_array_equal(got["seq"][:live][keep], acc[keep])
    if flags:
        assert got["flags"] == want["flags"], (got["flags"], want["flags"])
    return got, want


# ---------------------------------------------------------------------------------------------------------------- the fold
@pytest.mark.parametrize("n_parts", N_PARTS)
def test_fold_alone_at_every_slice_count(L, n_parts):
    """zero weights and biases: nll = lse, held to the normaliser bar alone (the logit part of the bar is its atol at y = 0, 2e-5: taken
    out here)"""
    P = Problem([8, 36], 100, n_parts, zero_logit=True)
    want = run(FK, P, False, None, 0)
    got = run(L, P, True, None, 0)
    ref = want["tok"][:100]
    err = np.abs(got["tok"][:100] - ref)
    assert np.abs(ref).max() > 20.0                          # (the spread maxima made it to the result)
    assert (err <= 2e-6 * np.maximum(1.0, np.abs(ref))).all(), float(err.max())
    assert got["flags"] == 0
    MEASURED["fold"] = max(MEASURED["fold"], float((err / np.maximum(1.0, np.abs(ref))).max()))
    print("fold alone, n_parts = %d: largest error %.3g x max(1, |lse|); so far %.3g" % (n_parts, float(
        (err / np.maximum(1.0, np.abs(ref))).max()), MEASURED["fold"]))


@pytest.mark.parametrize("self_norm", [0, 1])
@pytest.mark.parametrize("n_parts", N_PARTS)
def test_slice_counts(L, n_parts, self_norm):
    check(L, Problem([200, 100, 52], 100, n_parts), None, self_norm)


# ---------------------------------------------------------------------------------------------------------------- rows
def _counts(bound):
    out = []
    for n in (None, 0, 1, bound - 1, bound, bound + 7):
        if n not in out:
            out.append(n)
    return out


@pytest.mark.parametrize("tok", [True, False], ids=["tok", "notok"])
@pytest.mark.parametrize("bound,n", [(b, n) for b in BOUNDS for n in _counts(b)],
                         ids=lambda v: "NULL" if v is None else str(v))
def test_row_bounds_and_device_counts(L, bound, n, tok):
    P = Problem([8, 36], bound, 9)
    check(L, P, n, 0, tok=tok)
    check(L, P, n, 1, tok=tok)


# ---------------------------------------------------------------------------------------------------------------- the logit
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_logit_alone_on_every_layout(L, layout):
    """self_norm: nll = -y, held to the logit bar alone"""
    P = Problem(LAYOUTS[layout], 100, 25)
    want = run(FK, P, False, None, 1)
    got = run(L, P, True, None, 1)
    ref = want["tok"][:100]
    err = np.abs(got["tok"][:100] - ref)
    assert (err <= 2e-5 + 2e-5 * np.abs(ref)).all(), float(err.max())
    rel = float((err / (1.0 + np.abs(ref))).max())
    MEASURED["logit"] = max(MEASURED["logit"], rel)
    print("logit alone, %s: largest error %.3g x (1 + |y|), |y| up to %.3g; so far %.3g" % (layout, rel, float(np.abs(ref).max()),
                                                                                          MEASURED["logit"]))


@pytest.mark.parametrize("self_norm", [0, 1])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts(L, layout, self_norm):
    P = Problem(LAYOUTS[layout], 100, 25)
    edges = {w for i in range(P.nseg) for w in (P.segs_c[i].v_start, P.segs_c[i].v_end - 1)}
    assert edges <= set(P.target[:100].tolist())
    check(L, P, None, self_norm)
    check(L, P, 99, self_norm, tok=False)


# ---------------------------------------------------------------------------------------------------------------- accumulation, flags
@pytest.mark.parametrize("self_norm", [0, 1])
def test_two_calls_accumulate(L, self_norm):
    P = Problem([200, 100, 52], 33, 9)
    check(L, P, None, self_norm, calls=2)
    check(L, P, 32, self_norm, calls=2)


@pytest.mark.parametrize("self_norm", [0, 1])
def test_flags_null(L, self_norm):
    """flags NULL: the launch completes, also with a target outside every segment on one row"""
    P = Problem([8, 36], 33, 9)
    check(L, P, None, self_norm, flags=False)
    tgt = P.target.copy()
    tgt[5] = -1
    got, want = check(L, P, None, self_norm, flags=False, skip=(5,), target=tgt)
    assert np.isnan(got["tok"][5]) and np.isnan(got["seq"][5])


@pytest.mark.parametrize("self_norm", [0, 1])
@pytest.mark.parametrize("bad", ["v_end", "minus_one", "both"])
def test_target_outside_every_segment(L, bad, self_norm):
    P = Problem([200, 100, 52], 40, 9)
    rows = {"v_end": {7: V}, "minus_one": {33: -1}, "both": {0: V, 39: -1}}[bad]
    tgt = P.target.copy()
    for r, w in rows.items():
        tgt[r] = w
    got, want = check(L, P, None, self_norm, skip=tuple(rows), target=tgt)
    assert got["flags"] == 2
    for r in rows:
        assert np.isnan(got["tok"][r]) and np.isnan(got["seq"][r]), r
    # a bad target on a row past the count is not looked at
    got, want = check(L, P, 33 if bad == "minus_one" else 0 if bad == "both" else 7, self_norm, target=tgt)
    assert got["flags"] == 0


@pytest.mark.parametrize("value", [np.inf, np.nan], ids=["inf", "nan"])
def test_non_finite_slice_sum(L, value):
    P = Problem([8, 36], 40, 9)
    part = P.part.copy()
    part[3, 17, 1] = value
    got, want = check(L, P, None, 0, skip=(17,), part=part)
    assert got["flags"] == 1
    assert not np.isfinite(got["tok"][17]) and not np.isfinite(got["seq"][17])
    # self_norm does not read the slices: no flag, every row right
    got, want = check(L, P, None, 1, part=part)
    assert got["flags"] == 0


def test_refused_arguments(L):
    P = Problem([8, 36], 4, 1)
    for lib, cuda in ((FK, False), (L, True)):
        call = lambda n_segs, ldt, n_rows: lib.jlm_score_fold(P.segs(cuda), n_segs, None, None, ldt, None, P.ld_part, 1, 0, None, None,
                                                              n_rows, None, None, None, None)
        assert call(0, P.ldt, 4) == -1
        assert call(9, P.ldt, 4) == -1
        assert call(2, P.ldt + 2, 4) == -1
        assert call(2, P.ldt, 0) == 0                       # no rows: nothing launched, nothing read


# ---------------------------------------------------------------------------------------------------------------- the header's claims
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_logit_is_edge_logits_bit_for_bit(L, layout):
    """"wordlist_kernel<0>'s f32 arithmetic": the same (row, word) through jlm_edge_logits -- one group per row, beam 1, a list of one
    word -- gives the same f32 bits as -nll of the self-normalised fold"""
    P = Problem(LAYOUTS[layout], 100, 1)
    n = P.bound
    got = run(L, P, True, None, 1)
    y_fold = (-got["tok"][:n]).astype(np.float32)
    assert (y_fold.astype(np.float64) == -got["tok"][:n]).all()          # the f64 nll is the f32 logit, widened
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    ar = np.arange(n, dtype=np.int32)
    T, b2, g0, cnt, cidx, wl, off, wl_idx, out = (t(x) for x in (P.T, P.b2, ar, np.ones(n, np.int32), ar, P.target[:n],
                                                                 np.arange(n + 1, dtype=np.int32), ar, ar))
    edge = t(np.full(n + 8, 5.0, dtype=np.float32))
    assert L.jlm_edge_logits(P.segs_g, P.nseg, b2.data_ptr(), T.data_ptr(), P.ldt, g0.data_ptr(), cnt.data_ptr(), cidx.data_ptr(),
                             wl.data_ptr(), off.data_ptr(), wl_idx.data_ptr(), 0, out.data_ptr(), edge.data_ptr(), 1, n, _st()) == 0
    torch.cuda.synchronize()
    e = edge.cpu().numpy()
    assert (e[n:] == 5.0).all()
    np.testing.assert_array_equal(y_fold.view(np.uint32), e[:n].view(np.uint32))


@pytest.mark.parametrize("n_parts", [1, 9, 25, 33, 96])
def test_fold_is_the_beam_steps_fold_bit_for_bit(L, n_parts):
    """"the beam step's fold": jlm_beam_step's fused combine (jlm_beam_state.lse_part) of the same slices leaves the same f64 bits in
    lse[] as the fold leaves in nll (zero weights and biases: nll = lse).  Frame 0 lists one row per sentence; the step of frame 1 folds
    the slices at those rows' live positions"""
    B, beam, F = 45, 1, 3
    Pb = _beam_problem(np.random.default_rng(n_parts), B, beam, F, 2)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    G, rmax = Pb["G"], Pb["rmax"]
    ints = {k: t(Pb[k]) for k in ("slen", "end_off", "nstart", "nword")}
    score, lse = t(np.zeros(G)), t(np.full(G, 1e30))
    edge = t(np.zeros(max(Pb["N"], 1) * beam, dtype=np.float32))
    bp, node, word = (t(np.full(G, -7, dtype=np.int32)) for _ in range(3))
    cnt, live, n_live = t(np.zeros(F * B, dtype=np.int32)), t(np.full(G, -1, dtype=np.int32)), t(np.zeros(F, dtype=np.int32))
    live_base = t(np.zeros(F * B, dtype=np.int32))
    P = Problem([4], rmax, n_parts, zero_logit=True, seed=1)
    part = t(P.part)
    lat = _lib.Lattice(B, beam, F, ints["slen"].data_ptr(), ints["end_off"].data_ptr(), ints["nstart"].data_ptr(), ints["nword"].data_ptr())
    st = _lib.BeamState(score.data_ptr(), lse.data_ptr(), None, bp.data_ptr(), node.data_ptr(), word.data_ptr(), cnt.data_ptr(),
                        live.data_ptr(), n_live.data_ptr(), edge.data_ptr(), live_base.data_ptr(), None, 0, 0)
    assert L.jlm_beam_step(lat, st, 0, 0, Pb["max_cands"], _st()) == 0
    st.lse_part, st.ld_part, st.n_parts = part.data_ptr(), P.ld_part, n_parts
    assert L.jlm_beam_step(lat, st, 1, 0, Pb["max_cands"], _st()) == 0
    torch.cuda.synchronize()
    nl = int(n_live[0].item())
    assert nl == B                                            # every sentence is longer than frame 0
    pos = live_base.cpu().numpy()[:B]
    assert sorted(pos.tolist()) == list(range(B))
    folded = lse.cpu().numpy()[np.arange(B) * beam]           # row g = s * beam of frame 0, folded from live position pos[s]
    got = run(L, P, True, None, 0)
    assert got["flags"] == 0
    np.testing.assert_array_equal(got["tok"][pos].view(np.uint64), folded.view(np.uint64))
