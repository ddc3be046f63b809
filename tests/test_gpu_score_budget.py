"""GPU: where the score error of a peaked model comes from, stage by stage (tests/score_budget.py has the definitions).

R = 24 sentences of 28-39 words are stepped through LSTM_Model.score_streams ONE step per call; the state the device holds after
every step is read back, and the difference between the device's per-token -log p and the float64 oracle's is split, exactly, into
drift (earlier steps' state error, propagated in exact arithmetic), gate (this step's LSTM step), tproj (its T projection), norm (its
normaliser) and logit (its f32 target logit).  The local stages also run through the numpy restatements of tests/fake_hip.py on host
copies of the device's own operands and stage inputs: their error is what the operand formats cost, the device's minus theirs what
the arithmetic costs.  One table per case (pytest -s; profiles/score_budget_gpu_tests.log keeps a run's).

Asserted:
  a. the identities: the five stages sum to nll_D - nll_O within 1e-12; lse_D - y_D gives the step's nll_tok back to one f64 ulp;
     the recomputed T is the step's own T and the stepped values are those of one model.score call, bit for bit;
  b. logit within the worst-case bound of its documented chain, from the data (score_budget.logit_bound);
  c. every local stage unbiased: |mean over the N tokens| <= 4 rms / sqrt(N) (drift is autocorrelated by nature: measured only) --
     for tproj and logit in every case, for gate and norm where it holds; where it does not (RECORDED) the stage's mean is held under
     half an f32 ulp of its own output instead (score_budget.Budget.half_ulp_caps), so no bias is open-ended;
  d. 8 streams x 400 steps: the per-token bar 1e-5 at every step; the rms of drift over steps 20-60 and 360-400 and their ratio are
     recorded, not asserted (nothing in the project yields a bar for a ratio).

The model is H = 512 with logits of +-20 (peaked20-*): the effect scales with both; mid-vtable is the flat-logit control, and one case
scores the words the oracle finds most likely -- the regime of real text, where E_p[y_T] - y_T(target) is near 0 and a common-mode
bias of h would vanish.

What the first run found (MI355X; before -> after the fix, per token):
  norm   on peaked20-vtable was -4.6e-7 on EVERY token (rms 4.9e-7: almost no spread), with mixed rows and split rows, random and
         likely targets alike, all of it arithmetic cost -- three quarters of a sentence's error (per-sentence rms 1.5e-5 of 2.0e-5).
         Cause: the bias column of split rows is multiplied by log2(e) held as f16 hi + lo, log2(e) (1 + 6.9e-8), so every word's bias
         was off by the same +7.2e-8 relative and the log-normaliser by E_p[b2] times that.  Fixed where the column is packed
         (jlm_amd/rowformats.py split_bias_correction; tests/test_gpu_split_logits.py::test_bias_column_carries_no_common_mode_error):
         norm mean -4.6e-7 -> -9.3e-8, per-sentence rms 1.5e-5 -> 3.2e-6; a sentence's total error, worst 2.9e-5 -> 1.5e-5, rms
         2.0e-5 -> 8.4e-6, and the per-sentence bar of tests/test_gpu_score.py holds.  What is left of norm is the same on every
         model and form that has logits of +-20 -- arithmetic cost -7.6e-8 ... -7.9e-8 on peaked20-vtable with mixed rows, with split
         rows, and on peaked20-tied, which has no bias column -- and 30 times smaller on mid-vtable: the f32 running sums of the
         normaliser kernels, which lose the terms below half an ulp of the sum (emulated in numpy on these logits: -1.4e-8 ... -9e-8
         with 64 ... 1 ranges per segment).  Recorded, under half an ulp of the log-normaliser (2.2e-7).
  gate   on the peaked20 models with random targets: -1.3e-7 (vtable), -3.5e-7 (tied), arithmetic cost; none with likely targets or on
         mid-vtable.  The device's h is 6e-8 (2^-24) smaller in magnitude than the restatement's from the same operands, common to
         all units: the signature of (E_p[y_T] - y_T(target)) d.  A third of the arithmetic part is the f32 constant log2(e) in the
         gates' exponent scale (-1.3e-8 on every pre-activation; emulated on the oracle: -5.9e-8 per token of -1.9e-7); the rest is the
         hardware exp2 / rcp of jlm_sigmoid_k / jlm_tanh_k, documented as 1 ulp each and not correctly rounded.  That is the
         instructions' documented accuracy: no kernel is changed for it here; it stays under half an ulp of h (1.9e-7 / 5.3e-7) and
         costs a 35-word sentence of random words 5e-6.
  tproj, logit: unbiased everywhere, logit within 7 % of its chain's worst-case bound.
  drift  does not grow: its rms over steps 360-400 is 1.05 x that over steps 20-60 (peaked20-vtable), 1.08 x (mid-vtable)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib, score as jscore                                   # noqa: E402
from tests import score_budget as sb                                        # noqa: E402
from tests.gpu_rows import load_model, oracle_lm                            # noqa: E402
from tests.test_gpu_kernels import _st, _unsplit                            # noqa: E402

pytestmark = pytest.mark.gpu

R, LO, HI = 24, 28, 39
TOK_ATOL = 1e-5                       # the per-token bar of tests/test_gpu_score.py
_MODELS = {}


def _load(fx, name, knob, monkeypatch):
    """the fixture's model (loaded under `knob`=0 if given) and its oracle, kept for the module"""
    if (name, knob) not in _MODELS:
        if knob:
            monkeypatch.setenv(knob, "0")
        f = fx(name)
        _MODELS[(name, knob)] = (load_model(f["root"]), oracle_lm(f["root"]))
    return _MODELS[(name, knob)]


def _seg_array(m):
    return (_lib.Segment * len(m.segments))(*[_lib.Segment(sg["v_start"], sg["v_end"], sg["k"], sg["t_off"], m.seg_B[i].data_ptr(), sg["ldb"])
                                              for i, sg in enumerate(m.segments)])


def device_steps(model, x, y, lens):
    """x, y [R, S] stepped one step per score_streams call -> (score_budget.Steps, raw host copies (h, c, T) for the restatements).
    Per step: the state read back; T recomputed from it with the launch the step itself makes (jlm_gemm_nt_split on the split rows,
    jlm_gemm_nt on plain f32 rows) and compared, bit for bit, with the T rows the step left; the device's target logit read from
    jlm_score_fold(self_norm = 1) on that T."""
    m, L = model.dev, _lib.lib()
    Rn, S = x.shape
    assert m.pmt is not None and not m.self_norm
    sets = []

    class Recording(jscore.RowSets):                                          # the call's buffers, kept: its T rows are the step's own
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            sets.append(self)

    segs = _seg_array(m)
    rows = torch.arange(Rn, dtype=torch.int32, device=m.device)
    nll, ylog = np.empty((S, Rn)), np.empty((S, Rn))
    hs, cs, Ts = [], [], []
    h = c = None
    orig, jscore.RowSets = jscore.RowSets, Recording
    try:
        for t in range(S):
            del sets[:]
            tok, h, c = model.score_streams(x[:, t:t + 1], y[:, t:t + 1], h, c)
            nll[t] = tok[:, 0]
            T = torch.zeros((Rn, m.ldt), dtype=torch.float32, device=m.device)
            with m._ctx():
                if m.split_lstm:
                    rc = L.jlm_gemm_nt_split(h.data_ptr(), m.H, rows.data_ptr(), m.pmt_split.data_ptr(), m.H, None, T.data_ptr(), m.ldt,
                                             rows.data_ptr(), None, float(m.t_descale), Rn, m.pmt.shape[0], m.H, None, _st())
                else:
                    rc = L.jlm_gemm_nt(h.data_ptr(), m.H, rows.data_ptr(), m.pmt.data_ptr(), m.H, None, T.data_ptr(), m.ldt, rows.data_ptr(),
                                       None, Rn, m.pmt.shape[0], m.H, None, _st())
                assert rc == 0, rc
                tg = torch.as_tensor(np.ascontiguousarray(y[:, t], dtype=np.int32)).to(m.device)
                seq = torch.zeros(Rn, dtype=torch.float64, device=m.device)
                yk = torch.zeros(Rn, dtype=torch.float64, device=m.device)
                fl = torch.zeros(1, dtype=torch.int32, device=m.device)
                assert L.jlm_score_fold(segs, len(m.segments), m.b2.data_ptr(), T.data_ptr(), m.ldt, None, Rn, 0, 1, tg.data_ptr(), None, Rn,
                                        seq.data_ptr(), yk.data_ptr(), fl.data_ptr(), _st()) == 0
                torch.cuda.synchronize()
            assert int(fl.cpu()[0]) == 0
            assert len(sets) == 1 and torch.equal(sets[0].T.view(torch.int32)[:, :m.pmt.shape[0]], T.view(torch.int32)[:, :m.pmt.shape[0]]), \
                "the recomputed T is not the step's own (step %d)" % t
            ylog[t] = -yk.cpu().numpy()
            hs.append(h.detach().cpu().clone())
            cs.append(c.detach().cpu().clone())
            Ts.append(T.cpu())
    finally:
        jscore.RowSets = orig
    h_raw, c_raw, T_raw = torch.stack(hs), torch.stack(cs), torch.stack(Ts)
    if m.split_lstm:
        h64 = (_unsplit(h_raw.reshape(S * Rn, m.H)) / m.h_scale).reshape(S, Rn, m.H)
    else:
        h64 = h_raw.numpy().astype(np.float64)
    st = sb.Steps(x, y, lens, nll, h64, c_raw.numpy().astype(np.float64), T_raw.numpy().astype(np.float64), ylog)
    return st, (h_raw, c_raw, T_raw)


def _check_layout(m, lm):
    offs, ldt = sb.t_layout(lm)
    assert ldt == m.ldt and [o for o, _s in offs] == [sg["t_off"] for sg in m.segments]


def _budget(model, lm, x, y, lens, title):
    m = model.dev
    _check_layout(m, lm)
    st, (h_raw, c_raw, T_raw) = device_steps(model, x, y, lens)
    restated = sb.restate(m, x, y, h_raw, c_raw, T_raw) if m.split_lstm and m.split_array is not None else None
    b = sb.decompose(lm, st, restated)                                        # a: the identities
    live = np.arange(x.shape[1])[:, None] < lens[None, :]
    rows = "mixed rows (%s)" % m.mixed_fmt if m.mixed is not None else "split rows" if m.split_array is not None else "f32 rows"
    print()
    print(sb.table("%s, normaliser on %s" % (title, rows), b))
    if restated is not None:
        # the common-mode part of the device's own state and T against the restatement's: the least-squares d of dev = (1 + d) restated
        fit = lambda dev, ref: float((((dev - ref) * ref)[live]).sum() / ((ref * ref)[live]).sum())
        print("  common-mode relative error against the restatement: h %+.2e, T %+.2e; mean of T_D - T_R %+.2e (rms of T %.2g)"
              % (fit(st.h, restated["h"]), fit(st.T, restated["T"]), float((st.T - restated["T"])[live].mean()),
                 float(np.sqrt((st.T[live] ** 2).mean()))))
    return b, st, live


# c, where it does not hold: (case, stage) -> the measured mean per token (MI355X, profiles/score_budget_gpu_tests.log).  These stages'
# errors share a sign; what they are is in the module docstring.  They are held under score_budget.Budget.half_ulp_caps instead: a
# same-signed error below half an f32 ulp of the stage's own output.
RECORDED = {
    "peaked20-vtable, random targets": dict(gate=-1.32e-7, norm=-9.3e-8),
    "peaked20-vtable (JLM_LSE_MIXED=0), random targets": dict(gate=-1.32e-7, norm=-1.05e-7),
    "peaked20-tied, random targets": dict(gate=-3.52e-7, norm=-8.8e-8),
    "mid-vtable, random targets": dict(norm=-2.5e-9),
    "peaked20-vtable, likely targets": dict(norm=-1.52e-7),
}


def _assert_stages(b, title):
    worst = float((np.abs(b.dev["logit"]) / b.bound).max())
    print("  logit: largest error %.3g of the chain's worst-case bound" % worst)
    assert (np.abs(b.dev["logit"]) <= b.bound).all(), (title, worst)         # b
    assert np.abs(b.total).max() <= TOK_ATOL, (title, float(np.abs(b.total).max()))
    caps = b.half_ulp_caps()
    for s in sb.LOCAL:                                                        # c
        ok, mean, bar = sb.unbiased(b.dev[s])
        if s in RECORDED[title]:
            print("  %s: errors share a sign -- mean %+.3g against 4 rms / sqrt(N) = %.3g (recorded %+.3g); half an ulp: %.3g"
                  % (s, mean, bar, RECORDED[title][s], caps[s]))
            assert abs(mean) <= caps[s], (title, s, mean, caps[s])
        else:
            assert ok, (title, s, "errors share a sign: mean, 4 rms / sqrt(N)", mean, bar)


def _random_sentences(V, seed):
    rng = np.random.RandomState(seed)
    return [list(rng.randint(1, V, size=L)) for L in rng.randint(LO, HI + 1, size=R)]


@pytest.mark.parametrize("name,knob", [("peaked20-vtable", None), ("peaked20-vtable", "JLM_LSE_MIXED"), ("peaked20-tied", None),
                                       ("mid-vtable", None)])
def test_stage_budget_random_targets(name, knob, fx, monkeypatch):
    model, lm = _load(fx, name, knob, monkeypatch)
    assert model.dev.H == 512 and (not knob or model.dev.mixed is None)
    seqs = _random_sentences(model.dev.V, 11)
    x, y, lens = sb.sentence_steps(seqs, 1)
    title = "%s%s, random targets" % (name, " (%s=0)" % knob if knob else "")
    b, st, live = _budget(model, lm, x, y, lens, title)
    # the stepped values are those of one call, bit for bit (ragged rows padded, steps past a sentence's length ignored)
    one = model.score(seqs, 1)
    for r, g in enumerate(one):
        assert np.array_equal(st.nll[:lens[r], r], g), (title, r)
    _assert_stages(b, title)


def test_stage_budget_likely_targets(fx, monkeypatch):
    """every next word the oracle's argmax (distinct first words, so the sentences differ): E_p[y_T] - y_T(target) is near 0"""
    model, lm = _load(fx, "peaked20-vtable", None, monkeypatch)
    lens = np.random.RandomState(12).randint(LO, HI + 1, size=R)
    start = np.random.RandomState(13).choice(np.arange(2, model.dev.V), size=R, replace=False)
    seqs = sb.chosen_sentences(lm, start, lens, np.argmax)
    x, y, lens = sb.sentence_steps(seqs, 1)
    x[:, 0] = start
    title = "peaked20-vtable, likely targets"
    b, st, live = _budget(model, lm, x, y, lens, title)
    whole, _h, _c = model.score_streams(x, y)                                 # (score() starts every row from one word: the stream form)
    assert np.array_equal(whole.T[live], st.nll[live]), title
    _assert_stages(b, title)


@pytest.mark.parametrize("name", ["peaked20-vtable", "mid-vtable"])
def test_long_horizon(name, fx, monkeypatch):
    """d: 8 streams x 400 steps, one step per call, state carried"""
    model, lm = _load(fx, name, None, monkeypatch)
    B, S = 8, 400
    rng = np.random.RandomState(14)
    w = rng.randint(1, model.dev.V, size=(B, S + 1))
    x, y = w[:, :-1], w[:, 1:]
    x[:, 0] = 1
    lens = np.full(B, S)
    st, _raw = device_steps(model, x, y, lens)
    ti, ri = np.nonzero(np.ones((S, B), dtype=bool))
    tgt = y[ri, ti]
    nll_of = lambda X: np.subtract(*sb.lse_and_target(lm.project, X, tgt))
    nll_o = nll_of(sb.oracle_run(lm, x)[ti, ri])
    zero = np.zeros((1, B, lm.hidden_size))
    h_star, _c = lm.lstm_cell(x[ri, ti], np.concatenate([zero, st.h[:-1]])[ti, ri], np.concatenate([zero, st.c[:-1]])[ti, ri])
    drift = (nll_of(h_star) - nll_o).reshape(S, B)
    total = st.nll - nll_o.reshape(S, B)
    rms = lambda e: float(np.sqrt(np.mean(e * e)))
    early, late = rms(drift[20:60]), rms(drift[360:400])
    print("\n%s, 8 streams x 400 steps: |nll_D - nll_O| max %.3g (step %d), rms %.3g; drift rms steps 20-60 %.3g, steps 360-400 %.3g, ratio %.2f;"
          " total rms steps 20-60 %.3g, 360-400 %.3g; mean of total %.3g"
          % (name, float(np.abs(total).max()), int(np.abs(total).max(axis=1).argmax()), rms(total), early, late, late / early,
             rms(total[20:60]), rms(total[360:400]), float(total.mean())))
    assert np.abs(total).max() <= TOK_ATOL, float(np.abs(total).max())
