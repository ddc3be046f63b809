"""GPU: the continuous cache end to end (LSTM_Model.score_streams_cached / score_cached, python -m jlm_amd.perplexity --cache; csrc
jlm_score_cache_frames + cache_rows_kernel) against the float64 definition (jlm_amd.cache.cache_log_probs) over the oracle's own
states (OracleLM.lstm_cell, oracle/jlm_oracle.py).

The bar of a position is computed here from what the device returned, not a constant: the kernel's derived bar (tests/cache_budget.py;
derivation in tests/test_gpu_cache_rows.py) plus what the difference D between the device's states and the oracle's can move a
score, theta (|Dq . k| + |q . Dk| + |Dq . Dk|), maximised over the position's window.  The device's states are
CachedScores.state.numpy() of a call with N >= the stream's length.  nll_lm must be score_streams' bits."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import cache as C, config as jconfig                                           # noqa: E402
from tests.cache_budget import kernel_bar                                                   # noqa: E402
from tests.gpu_rows import UNTIED_F32, fixture_model, lse, oracle_lm                        # noqa: E402

pytestmark = pytest.mark.gpu

MODELS = ["small-tied", "small-vtable", "small-tied-sn", "odd-tied", UNTIED_F32]
THETAS = [0.0, 0.5, 2.0]
TOK_ATOL = 1e-5                                                                              # tests/test_gpu_score.py's bar on nll


def _stream(V, B=3, n=45, seed=11):
    """B streams of n steps over a pool of a dozen words: matches and misses both occur"""
    rng = np.random.RandomState(seed)
    pool = rng.randint(2, V, size=12)
    s = pool[rng.randint(0, 12, size=(B, n + 1))].astype(np.int32)
    return s[:, :-1], s[:, 1:]


def oracle_states(lm, x, y):
    """-> (h [B, n, H] float64: the state each step leaves, nll [B, n] float64) of streams from the zero state"""
    B, n = x.shape
    h, c = lm.zero_state(B)
    hs, nll = [], []
    sn = lm.config["self_norm"]
    for t in range(n):
        h, c = lm.lstm_cell(x[:, t], h, c)
        yy = lm.project(h)
        yt = yy[np.arange(B), y[:, t]]
        nll.append(-yt if sn else lse(yy) - yt)
        hs.append(np.array(h, dtype=np.float64))
    return np.stack(hs, axis=1), np.stack(nll, axis=1)


def position_bars(dev_h, ora_h, words, N, thetas, split):
    """[n_theta, n]: the bar of every position of ONE row -- kernel_bar over the device's operands plus theta (|Dq.k| + |q.Dk| + |Dq.Dk|)
    maximised over the window; 0 where the definition is exact (-inf)"""
    n, H = ora_h.shape
    D = dev_h - ora_h
    out = np.zeros((len(thetas), n))
    for q in range(1, n):
        lo = max(q - N, 0)
        same = words[lo:q] == words[q]
        if not same.any():
            continue
        k, dk = ora_h[lo:q], D[lo:q]
        move = float((np.abs(k @ D[q]) + np.abs(dk @ ora_h[q]) + np.abs(dk @ D[q])).max())
        A = float((np.abs(dev_h[lo:q]) @ np.abs(dev_h[q])).max())
        dot = k @ ora_h[q]
        for t, theta in enumerate(thetas):
            s = theta * dot
            m = s.max()
            logZ, logM = np.log(np.exp(s - m).sum()), np.log(np.exp(s[same] - m).sum())
            out[t, q] = kernel_bar(split, H, N, theta, A, logM, logZ) + theta * move
    return out


def _run_cut(model, x, y, spec, cuts, plain=False):
    h = c = state = None
    hp = cp = None
    parts, at = [], 0
    for k in cuts:
        res = model.score_streams_cached(x[:, at:at + k], y[:, at:at + k], spec, h, c, state)
        if plain:                                                          # the same input through score_streams: the same bits
            nll, hp, cp = model.score_streams(x[:, at:at + k], y[:, at:at + k], hp, cp)
            assert nll.tobytes() == res.nll_lm.tobytes() and nll.dtype == res.nll_lm.dtype == np.float64
            assert torch.equal(hp.view(torch.int32), res.h.view(torch.int32)) and torch.equal(cp, res.c)
        h, c, state = res.h, res.c, res.state
        parts.append(res)
        at += k
    return parts, (np.concatenate([p.nll_lm for p in parts], axis=1), np.concatenate([p.logp_cache for p in parts], axis=2),
                   np.concatenate([p.n_entries for p in parts], axis=1))


@pytest.mark.parametrize("name", MODELS)
def test_streams_match_the_definition(name, fx, monkeypatch):
    f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    lm = oracle_lm(f["root"])
    x, y = _stream(m.V)
    B, n = x.shape
    ora_h, ora_nll = oracle_states(lm, x, y)
    # the device's own states: one call that keeps them all
    full = model.score_streams_cached(x, y, C.CacheSpec(64, theta=THETAS))
    dev_h, words, pos = full.state.numpy()
    assert dev_h.shape == (B, n, m.H) and np.array_equal(words, y) and np.array_equal(pos, np.arange(n)) and full.state.pos == n
    dev_h = dev_h.astype(np.float64)
    print("%s: max |h_dev - h_oracle| %.3e" % (name, np.abs(dev_h - ora_h).max()))
    np.testing.assert_allclose(full.nll_lm, ora_nll, rtol=0, atol=TOK_ATOL)
    for N in (16, 64):
        spec = C.CacheSpec(N, theta=THETAS, lam=0.2)
        parts, (nll, lpc, cnt) = _run_cut(model, x, y, spec, [20, 20, 5], plain=True)
        assert np.array_equal(cnt, np.broadcast_to(np.minimum(np.arange(n), N), (B, n)))
        assert parts[-1].state.count == min(n, N) and parts[-1].state.pos == n
        worst = 0.0
        bars = np.zeros((len(THETAS), B, n))
        for b in range(B):
            want, wc = C.cache_log_probs(ora_h[b], y[b], N, THETAS)
            bars[:, b] = position_bars(dev_h[b], ora_h[b], y[b], N, THETAS, bool(m.split_lstm))
            assert np.array_equal(wc, cnt[b])
            assert np.array_equal(np.isneginf(want), np.isneginf(lpc[:, b])) and not np.isnan(lpc[:, b]).any(), (name, N, b)
            ok = np.isfinite(want)
            err = np.abs(lpc[:, b][ok] - want[ok])
            worst = max(worst, float((err / bars[:, b][ok]).max()))
            assert np.all(err <= bars[:, b][ok]), (name, N, b, float(err.max()))
        fin = np.isfinite(lpc)
        assert fin.any() and np.isneginf(lpc[:, :, 1:]).any()
        print("%s N %d: %d finite lpc, max err / bar %.3f, largest bar %.3e" % (name, N, int(fin.sum()), worst, bars.max()))
        # another cut of the stream: the same windows, summed in another order -- within the kernel's part of the bar
        for cuts in ([45], [7, 38]):
            _p, (nll2, lpc2, cnt2) = _run_cut(model, x, y, spec, cuts)
            assert np.allclose(nll2, nll, rtol=0, atol=TOK_ATOL)
            assert np.array_equal(cnt2, cnt) and np.array_equal(np.isneginf(lpc2), np.isneginf(lpc))
            kb = np.zeros_like(bars)
            for b in range(B):
                kb[:, b] = position_bars(dev_h[b], dev_h[b], y[b], N, THETAS, bool(m.split_lstm))        # D = 0: the kernel bar alone
            print("%s N %d cut %s: max |lpc - lpc'| / kernel bar %.3f" % (name, N, cuts, float((np.abs(lpc2[fin] - lpc[fin]) / kb[fin]).max())))
            assert np.all(np.abs(lpc2[fin] - lpc[fin]) <= kb[fin]), (name, N, cuts)
        # the mixture on the host: nll(0) is nll_lm's bits
        assert all(p.nll(0).tobytes() == p.nll_lm.tobytes() for p in parts)


@pytest.mark.parametrize("name", ["small-tied", UNTIED_F32])
def test_score_cached_ragged_sequences(name, fx, monkeypatch):
    """ragged sequences, empty ones included, each from an empty cache: the mixed -log p against the definition over the oracle's
    states and -log p.  logaddexp is 1-Lipschitz in the larger of its arguments' errors: bar = nll's bar + lpc's bar"""
    f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    lm = oracle_lm(f["root"])
    rng = np.random.RandomState(2)
    pool = rng.randint(2, m.V, size=6)
    seqs = [[int(w) for w in pool[rng.randint(0, 6, size=L)]] for L in (9, 0, 30, 1, 17, 0, 30)]
    spec = C.CacheSpec(8, theta=0.7, lam=0.25)
    got = model.score_cached(seqs, 1, spec)
    assert [len(g) for g in got] == [len(s) for s in seqs] and all(g.dtype == np.float64 for g in got)
    plain = model.score(seqs, 1)
    for max_rows in (None, 2):
        if max_rows:
            got = model.score_cached(seqs, 1, spec, max_rows=max_rows)
        for s, g, p in zip(seqs, got, plain):
            if not len(s):
                continue
            x, y = np.array([[1] + s[:-1]]), np.array([s])
            ora_h, ora_nll = oracle_states(lm, x, y)
            dev = model.score_streams_cached(x, y, C.CacheSpec(64, theta=0.7))
            dev_h = dev.state.numpy()[0][0].astype(np.float64)
            want_lpc, cnt = C.cache_log_probs(ora_h[0], y[0], spec.size, spec.thetas)
            want = C.mix_nll(ora_nll[0], want_lpc[0], cnt, spec.lam)
            bar = TOK_ATOL + position_bars(dev_h, ora_h[0], y[0], spec.size, spec.thetas, bool(m.split_lstm))[0]
            assert np.all(np.abs(g - want) <= bar), (name, max_rows, len(s), float(np.abs(g - want).max()))
            if not max_rows:
                assert g[0] == p[0]                                        # an empty cache: the model's own bits, in score()'s row plan


def test_perplexity_command_line_with_cache(fx, tmp_path, capsys):
    """--cache prints the plain perplexity and the cached one; both equal a host computation from CachedScores"""
    from jlm_amd import perplexity
    from jlm_amd.data import Vocab
    from jlm_amd.score import stream_layout
    from tests.gpu_rows import load_model
    f = fx("small-vtable")
    jconfig.set_root(f["root"])
    vocab = Vocab(f["cfg"]["vocab_size"])
    words = [w for w in vocab.w2i if w not in ("<unk>", "<eos>")]
    rng = np.random.RandomState(8)
    passage = " ".join(words[i] for i in rng.choice(len(words), size=29, replace=False))
    path = str(tmp_path / "passage.txt")
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join([passage] * 12) + "\n")
    args = ["--root", f["root"], "-e", "1", "--mode", "stream", "-b", "4", "--num_steps", "5", "--file", path]
    plain = perplexity.main(args)
    out_plain = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Test perplexity")]
    got = perplexity.main(args + ["--cache", "40", "--theta", "0.5", "--lam", "0.2"])
    out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Test perplexity")]
    assert got == plain and out_plain == [out[0]] == ["Test perplexity: {}".format(plain)] and len(out) == 2
    cached = float(out[1].rsplit(" ", 1)[1])
    model = load_model(f["root"])
    sents, _unk = perplexity.encode_lines(perplexity.read_lines(path), vocab)
    x, y = stream_layout([i for s in sents for i in s], 4, 5)
    spec = C.CacheSpec(40, 0.5, 0.2)
    h = c = state = None
    tot = mix = 0.0
    for i in range(x.shape[1] // 5):
        res = model.score_streams_cached(x[:, 5 * i:5 * i + 5], y[:, 5 * i:5 * i + 5], spec, h, c, state)
        h, c, state = res.h, res.c, res.state
        p = np.where(res.n_entries > 0, 0.8 * np.exp(-res.nll_lm) + 0.2 * np.exp(res.logp_cache[0]), np.exp(-res.nll_lm))
        tot += res.nll_lm.sum()
        mix += -np.log(p).sum()
    np.testing.assert_allclose(plain, np.exp(tot / x.size), rtol=1e-12)
    np.testing.assert_allclose(cached, np.exp(mix / x.size), rtol=1e-10)
    assert cached < plain                                                  # a repeated passage: the cache helps


def test_state_of_another_model_or_row_count_is_refused(fx, monkeypatch):
    _f, model = fixture_model(fx, "small-tied", monkeypatch)
    _f2, other = fixture_model(fx, "small-vtable", monkeypatch)
    x, y = _stream(model.dev.V, n=6)
    spec = C.CacheSpec(4)
    res = model.score_streams_cached(x, y, spec)
    with pytest.raises(ValueError, match="another model"):
        other.score_streams_cached(x, y, spec, state=res.state)
    with pytest.raises(ValueError, match="streams"):
        model.score_streams_cached(x[:2], y[:2], spec, state=res.state)
