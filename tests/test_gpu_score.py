"""GPU: teacher-forced scoring (LSTM_Model.score / score_streams, python -m jlm_amd.perplexity; csrc jlm_score_frames +
score_fold_kernel) against the oracle's explicit-state OracleLM.predict arithmetic in float64 (oracle/jlm_oracle.py, pinned to the
reference's vectors at 1e-10 by tests/test_oracle_golden.py), and against LSTM_Model.evaluate.

Bars: per token |nll - oracle| <= 1e-5; per sentence the decode's path-score bar min(2e-5, 1e-6 (L + 1) + 2e-6); corpus perplexity
within a relative 1e-5 -- on every fixture, peaked20-vtable included (its expected failure is gone: tests/test_gpu_score_budget.py)."""
import os
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib, config as jconfig, rowsets, synth      # noqa: E402
from tests.gpu_rows import UNTIED_F32, fixture_model, load_model, lse, oracle_lm     # noqa: E402

pytestmark = pytest.mark.gpu

TOK_ATOL = 1e-5


def sent_atol(L):
    return min(2e-5, 1e-6 * (L + 1) + 2e-6)


def oracle_nll(lm, seqs, start, h=None, c=None):
    """per-sequence float64 -log p, all sequences stepped together (OracleLM.lstm_cell / project = OracleLM.predict's arithmetic;
    model.py:117-119: -y for self-normalised models).  h, c: the state to continue (rows = sequences); -> (nll list, h, c)"""
    R = len(seqs)
    lens = np.array([len(s) for s in seqs])
    if h is None:
        h, c = lm.zero_state(R)
    h, c = h.copy(), c.copy()
    out = [np.zeros(L) for L in lens]
    words = np.full(R, start, dtype=np.int64) if np.ndim(start) == 0 else np.asarray(start, dtype=np.int64).copy()
    sn = lm.config["self_norm"]
    for t in range(int(lens.max()) if R else 0):
        idx = np.nonzero(lens > t)[0]
        hl, cl = lm.lstm_cell(words[idx], h[idx], c[idx])
        h[idx], c[idx] = hl, cl
        y = lm.project(hl)
        tgt = np.array([seqs[r][t] for r in idx])
        yt = y[np.arange(len(idx)), tgt]
        nll = -yt if sn else lse(y) - yt
        for j, r in enumerate(idx):
            out[r][t] = nll[j]
        words[idx] = tgt
    return out, h, c


def _ragged(n, V, seed, lo=0, hi=40):
    rng = np.random.RandomState(seed)
    lens = rng.randint(lo, hi + 1, size=n)
    return [list(rng.randint(1, V, size=L)) for L in lens]


def _check(got, want, tag):
    """the three bars, asserted"""
    tot_g = tot_w = 0.0
    n_tok = 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (tag, i)
        if len(w):
            np.testing.assert_allclose(g, w, rtol=0, atol=TOK_ATOL, err_msg="%s row %d" % (tag, i))
            assert abs(g.sum() - w.sum()) <= sent_atol(len(w)), (tag, i, g.sum() - w.sum())
        tot_g += g.sum()
        tot_w += w.sum()
        n_tok += len(w)
    if n_tok:
        np.testing.assert_allclose(np.exp(tot_g / n_tok), np.exp(tot_w / n_tok), rtol=1e-5, err_msg=tag)


SMALL = ["small-tied", "small-untied", "small-dsoftmax", "small-vtable", "small-tied-sn", "small-vtable-sn",
         "wide-vtable", "wide-dsoftmax", "wideh-vtable", "wide128-tied"]
# V = 2 003 cut at 501 / 1 203 (jlm_amd/synth.py): no segment starts at, and the vocabulary does not end on, a multiple of 4
ODD = ["odd-tied", "odd-untied", "odd-dsoftmax", "odd-vtable", "odd-tied-sn", "odd-vtable-sn", "oddw-vtable"]
ODD_UNTIED_F32 = "odd-untied@f32"
ODD_EDGES = (0, 500, 501, 1202, 1203, 2002)         # the first and last word of every segment of the odd fixtures


def _on_edges(seqs):
    """the sequences with their first and last words moved onto the segment edges of the odd fixtures, every pair of them in turn: a
    word is the target of one step and the input of the next"""
    out = []
    for i, s in enumerate(seqs):
        s = list(s)
        if s:
            s[-1] = ODD_EDGES[(i // 6) % 6]
            s[0] = ODD_EDGES[i % 6]
        out.append(s)
    return out


@pytest.mark.parametrize("name", SMALL + [UNTIED_F32] + ODD + [ODD_UNTIED_F32])
def test_score_matches_oracle(name, fx, monkeypatch):
    f, model = fixture_model(fx, name, monkeypatch)
    lm = oracle_lm(f["root"])
    V = model.dev.V
    seqs = _ragged(300, V, seed=7)
    start = 1
    if name.startswith("odd"):
        assert V == 2003 and (name != ODD_UNTIED_F32 or rowsets.t_is_state(model.dev))
        seqs = _on_edges(seqs)
    if name == "oddw-vtable":                        # the 200 / 100 / 52 segments are there for the mixed / mx6 rows
        assert model.dev.mixed_idx == [0, 1, 2] or os.environ.get("JLM_LSE_MIXED") == "0" or os.environ.get("JLM_PRECISION") == "f32"
    got = model.score(seqs, start)
    assert isinstance(got, list) and all(g.dtype == np.float64 for g in got)
    want, _h, _c = oracle_nll(lm, seqs, start)
    _check(got, want, name)
    # one row, several calls (max_rows cuts the live prefix across calls), sums only
    one = model.score(seqs[:1], start)
    np.testing.assert_allclose(one[0], want[0], rtol=0, atol=TOK_ATOL)
    sums = model.score(seqs, start, per_token=False, max_rows=64)
    np.testing.assert_allclose(sums, [w.sum() for w in want], rtol=0, atol=2e-5)


@pytest.mark.parametrize("name,knob", [("mid-vtable", None), ("mid-untied", None), ("peaked20-vtable", None),
                                       ("peaked20-vtable", "JLM_LSE_MIXED")])
def test_score_full_size_call_against_oracle_sample(name, knob, fx, monkeypatch):
    """> 2 560 rows in one call: the live prefix shrinks across row tiles of every kernel; the oracle checks a sample of rows.
    peaked20 (logits of +-20, a trained model's statistics) used to miss the per-sentence bar on 5-6 of the 24 sampled sentences by up
    to 30 %, with mixed rows and split rows alike, and was reported as an expected failure.  tests/test_gpu_score_budget.py found the
    stage -- the normaliser: every bias of the split rows' bias column off by the same 7e-8 relative -- and with that fixed
    (rowformats.split_bias_correction) the bar holds, the worst sampled sentence at 1.26e-5 of 2e-5: asserted for every sentence,
    like everywhere else."""
    if knob:
        monkeypatch.setenv(knob, "0")
    f = fx(name)
    model = load_model(f["root"])
    V = model.dev.V
    seqs = _ragged(2700, V, seed=11)
    got = model.score(seqs, 1)
    assert model.dev.V == V and len(got) == 2700
    sample = list(range(0, 2700, 113))
    lm = oracle_lm(f["root"])
    want, _h, _c = oracle_nll(lm, [seqs[i] for i in sample], 1)
    for i, g, w in zip(sample, [got[i] for i in sample], want):
        if len(w):
            print("%s %s row %d, %d words: sentence error %+.3g of %.3g" % (name, knob, i, len(w), g.sum() - w.sum(), sent_atol(len(w))))
    _check([got[i] for i in sample], want, (name, knob))


@pytest.mark.parametrize("knob,value", [("JLM_LSE_MIXED", "0"), ("JLM_LSE_MX6", "0"), ("JLM_MX_FIXREF", "0"), ("JLM_PRECISION", "f32")])
@pytest.mark.parametrize("name", ["wide-vtable", "wide128-tied"])
def test_score_forced_forms(name, knob, value, fx, monkeypatch):
    monkeypatch.setenv(knob, value)
    f = fx(name)
    model = load_model(f["root"])
    if knob == "JLM_LSE_MIXED":
        assert not model.dev.mixed_idx
    if knob == "JLM_PRECISION":
        assert not model.dev.split_lstm and model.dev.split_array is None
    seqs = _ragged(300, model.dev.V, seed=3)
    want, _h, _c = oracle_nll(oracle_lm(f["root"]), seqs, 1)
    _check(model.score(seqs, 1), want, (name, knob))


def test_score_agrees_with_evaluate(fx):
    f = fx("small-vtable")
    model = load_model(f["root"])
    seqs = _ragged(6, model.dev.V, seed=5, lo=0, hi=12)
    got = model.score(seqs, 1)
    for s, g in zip(seqs, got):
        np.testing.assert_allclose(g, model.evaluate(1, s), rtol=1e-4)


def test_alone_and_in_a_batch(fx):
    f = fx("wide-vtable")
    model = load_model(f["root"])
    seqs = _ragged(300, model.dev.V, seed=9, lo=1)
    batch = model.score(seqs, 1)
    for i in (0, 17, 299):
        np.testing.assert_allclose(model.score([seqs[i]], 1)[0], batch[i], rtol=0, atol=TOK_ATOL)


@pytest.mark.parametrize("start", ODD_EDGES)
def test_odd_vocabulary_rows_alone_and_in_a_batch(start, fx):
    """V = 2 003: calls of 1, 31, 32 and 33 rows (the fold's 32 rows per workgroup) give what the same rows give inside a call of 300;
    start words and targets on the first and last word of every segment"""
    f = fx("odd-vtable")
    model = load_model(f["root"])
    assert model.dev.V == 2003
    seqs = _on_edges(_ragged(300, 2003, seed=21, lo=1))
    batch = model.score(seqs, start)
    want, _h, _c = oracle_nll(oracle_lm(f["root"]), seqs[:33], start)
    _check(batch[:33], want, ("odd-vtable", start))
    for n in (1, 31, 32, 33):
        got = model.score(seqs[:n], start)
        assert len(got) == n
        for i in range(n):
            np.testing.assert_allclose(got[i], batch[i], rtol=0, atol=TOK_ATOL, err_msg="%d rows, row %d" % (n, i))


@pytest.mark.parametrize("name", ["small-vtable", "wide-vtable", "small-untied", "odd-vtable", "oddw-vtable", "odd-untied"])
def test_streams_carry_state(name, fx):
    f = fx(name)
    model = load_model(f["root"])
    rng = np.random.RandomState(2)
    B, n = 37, 12
    x = rng.randint(0, model.dev.V, size=(B, 2 * n))
    y = rng.randint(0, model.dev.V, size=(B, 2 * n))
    if name.startswith("odd"):                       # start words and targets on the segment edges, every pair of them
        x[:36, 0] = np.tile(ODD_EDGES, 6)
        y[:36, 0] = np.repeat(ODD_EDGES, 6)
        x[:36, n] = np.repeat(ODD_EDGES, 6)
        y[:36, 2 * n - 1] = np.tile(ODD_EDGES, 6)
    whole, hw, cw = model.score_streams(x, y)
    a, h, c = model.score_streams(x[:, :n], y[:, :n])
    b, h2, c2 = model.score_streams(x[:, n:], y[:, n:], h, c)
    assert np.array_equal(np.concatenate([a, b], axis=1), whole)         # bit-identical
    assert torch.equal(h2, hw) and torch.equal(c2, cw)
    # the oracle over the same streams, state carried
    lm = oracle_lm(f["root"])
    want = np.zeros((B, 2 * n))
    hh, cc = lm.zero_state(B)
    for t in range(2 * n):
        hh, cc = lm.lstm_cell(x[:, t], hh, cc)
        yy = lm.project(hh)
        want[:, t] = lse(yy) - yy[np.arange(B), y[:, t]]
    np.testing.assert_allclose(whole, want, rtol=0, atol=TOK_ATOL)
    np.testing.assert_allclose(np.exp(whole.mean()), np.exp(want.mean()), rtol=1e-5)


@pytest.mark.parametrize("name", ["small-vtable", "small-char"])
def test_perplexity_module(name, fx, capsys):
    from jlm_amd import perplexity
    from jlm_amd.data import CharVocab, Vocab
    from jlm_amd.score import stream_layout
    f = fx(name)
    V = f["cfg"]["vocab_size"]
    synth.write_test_corpus(f["root"], f["lexicon"], V, 40, words_per_sentence=6, seed=13, oov_every=4)
    jconfig.set_root(f["root"])
    vocab = (CharVocab if f["cfg"].get("char_rnn") else Vocab)(V)
    sents, _unk = perplexity.encode_lines(perplexity.read_lines(os.path.join(f["root"], "data", "test.txt")), vocab)
    eos = vocab.c2i["<eos>"] if isinstance(vocab, CharVocab) else vocab.w2i["<eos>"]
    lm = oracle_lm(f["root"])
    want_s, _h, _c = oracle_nll(lm, sents, eos)
    pp_s = np.exp(sum(w.sum() for w in want_s) / sum(len(s) for s in sents))
    got = perplexity.main(["--root", f["root"], "-e", "1", "--mode", "sentence"])
    assert "Test perplexity: {}".format(got) in capsys.readouterr().out
    np.testing.assert_allclose(got, pp_s, rtol=1e-5)
    # stream mode: corpus_iterator over the concatenated ids, 4 streams of 5-step chunks, state carried (run_epoch)
    x, y = stream_layout([i for s in sents for i in s], 4, 5)
    hh, cc = lm.zero_state(4)
    tot = 0.0
    for t in range(x.shape[1]):
        hh, cc = lm.lstm_cell(x[:, t], hh, cc)
        yy = lm.project(hh)
        tot += (lse(yy) - yy[np.arange(4), y[:, t]]).sum()
    got = perplexity.main(["--root", f["root"], "-e", "1", "--mode", "stream", "-b", "4", "--num_steps", "5"])
    assert "Test perplexity: {}".format(got) in capsys.readouterr().out
    np.testing.assert_allclose(got, np.exp(tot / x.size), rtol=1e-5)


def test_nonfinite_normaliser_raises(tmp_path, monkeypatch):
    """the fixed-reference normaliser (jlm_vocab_lse_mixed_fr) forced onto a model whose logits leave its range: the fold kernel
    raises the flag word and score() turns it into an error (as the decode does, tests/test_gpu_edge_cases.py)"""
    if os.environ.get("JLM_PRECISION", "f16x3") != "f16x3" or os.environ.get("JLM_LSE_MIXED", "1") == "0":
        pytest.skip("the suite is running without the mixed rows")
    monkeypatch.setenv("JLM_MIXED_MAX_LSE_RMS", "0")
    root = str(tmp_path / "wide-vtable")
    synth.build_fixture(root, "wide-vtable")
    wp = os.path.join(root, "train", "experiments", "1", "weights", "lstm_weights.pkl")
    with open(wp, "rb") as fh:
        w = pickle.load(fh)
    for key in list(w):
        if key.startswith("LM"):
            w[key] = [b * np.float32(600.0) for b in w[key]] if isinstance(w[key], list) else w[key] * np.float32(600.0)
    with open(wp, "wb") as fh:
        pickle.dump(w, fh)
    model = load_model(root)
    m = model.dev
    assert m.mixed_idx and not m.lse_fixed_ref
    seqs = _ragged(8, m.V, seed=4, lo=2, hi=9)
    ok = model.score(seqs, 1)                    # the running-maximum form copes with any range
    assert all(np.isfinite(g).all() for g in ok)
    m.lse_fixed_ref = 1
    with pytest.raises(_lib.JlmHipError, match="not finite"):
        model.score(seqs, 1)
