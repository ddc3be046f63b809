"""GPU: ranking and prediction under the continuous cache end to end (LSTM_Model.rank_streams_cached / rank_cached /
predict_next_cached; csrc jlm_rank_cache_frames, jlm_predict_cache_rows, cache_query_kernel, cache_mix_rows_kernel) against the float64
definition: jlm_amd.cache.mixed_logits over the oracle's logits (OracleLM.project) with jlm_amd.cache.cache_distribution over the
oracle's own states (OracleLM.lstm_cell), on the five models of tests/test_gpu_cache.py.

Every device rank must lie in the interval the oracle's mixed logits leave open (tests/rank_cases.py interval) at

    delta_q = 2 * rank_cases.DELTA + the position's cache bar

-- y' = logaddexp(y, L + log rho + lpc) is 1-Lipschitz in the larger of its two arguments' errors: one DELTA for the logit, one for L
(1-Lipschitz in the logits), and the cache bar on lpc: the kernels' derived bar (tests/cache_mix_budget.py Y_BAR, maximised over the
window's words) plus what the difference D between the device's states and the oracle's can move a score, theta (|Dq . k| + |q . Dk| +
|Dq . Dk|), as tests/test_gpu_cache.py position_bars takes it.  The bar is computed from what the device returned, not fixed."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import cache as C                                                              # noqa: E402
from tests import rank_cases as rc                                                          # noqa: E402
from tests.cache_mix_budget import lpc_bar, lse_bar, y_bar                                  # noqa: E402
from tests.gpu_rows import fixture_model, lse, oracle_lm                                    # noqa: E402
from tests.test_gpu_cache import MODELS, TOK_ATOL, _stream, position_bars                   # noqa: E402

pytestmark = pytest.mark.gpu

LAM = 0.2
THETAS = [0.5, 2.0]
CUTS = ([45], [20, 20, 5], [7, 38])
MAX_PREFIX = 3
TOP = 10


def oracle_run(lm, x):
    """-> (h [B, n, H] float64: the state each step leaves, y [B, n, V] float64: its logits) of streams from the zero state"""
    B, n = x.shape
    h, c = lm.zero_state(B)
    hs, ys = [], []
    for t in range(n):
        h, c = lm.lstm_cell(x[:, t], h, c)
        ys.append(np.array(lm.project(h), dtype=np.float64))
        hs.append(np.array(h, dtype=np.float64))
    return np.stack(hs, axis=1), np.stack(ys, axis=1)


def mix_bars(dev_h, ora_h, words, ys, ymix, N, theta, lam, split, self_norm):
    """[n]: the cache bar of every position of ONE row (module docstring); 0 where the window is empty"""
    n, H = ora_h.shape
    D = dev_h - ora_h
    log_rho = np.log(lam) - np.log1p(-lam)
    out = np.zeros(n)
    for q in range(1, n):
        lo = max(q - N, 0)
        k, dk, ww = ora_h[lo:q], D[lo:q], words[lo:q]
        move = float((np.abs(k @ D[q]) + np.abs(dk @ ora_h[q]) + np.abs(dk @ D[q])).max())
        A = float((np.abs(dev_h[lo:q]) @ np.abs(dev_h[q])).max())
        s = theta * (k @ ora_h[q])
        e = np.exp(s - s.max())
        logZ = np.log(e.sum())
        L = 0.0 if self_norm else float(lse(ys[q]))
        L_b = lse_bar(ys[q], self_norm)
        for w in np.unique(ww):
            logc = np.log(e[ww == w].sum())
            b = lpc_bar(split, H, N, theta, A, logc, logZ) + theta * move
            out[q] = max(out[q], y_bar(b, L_b, L, log_rho, logc - logZ, ys[q][w], ymix[q][w]))
    return out


def run_cut(model, x, y, spec, cuts, top=TOP):
    h = c = state = None
    parts, at = [], 0
    for k in cuts:
        res = model.rank_streams_cached(x[:, at:at + k], y[:, at:at + k], spec, h, c, state, max_prefix=MAX_PREFIX, top=top)
        h, c, state = res.h, res.c, res.state
        parts.append(res)
        at += k
    return parts


def joined(parts):
    return (np.concatenate([p.ranks for p in parts], axis=1), np.concatenate([p.top_ids for p in parts], axis=1),
            np.concatenate([p.top_logp for p in parts], axis=1), np.concatenate([p.n_entries for p in parts], axis=1))


@pytest.mark.parametrize("name", MODELS)
def test_streams_rank_inside_the_oracles_interval(name, fx, monkeypatch):
    f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    lm = oracle_lm(f["root"])
    index = model.reading_index()
    x, y = _stream(m.V)
    B, n = x.shape
    sn = bool(m.self_norm)
    ora_h, ora_y = oracle_run(lm, x)
    plain_before = model.rank_streams(x, y, max_prefix=MAX_PREFIX)[0]
    # the device's own states: one scoring call that keeps them all
    dev_h = model.score_streams_cached(x, y, C.CacheSpec(64, theta=0.5)).state.numpy()[0].astype(np.float64)
    sets = {int(t): rc.level_sets(index, int(t), MAX_PREFIX) for t in np.unique(y)}
    for N in (16, 64):
        for theta in THETAS:
            spec = C.CacheSpec(N, theta=theta, lam=LAM)
            parts = run_cut(model, x, y, spec, CUTS[1])
            ranks, top_ids, top_logp, cnt = joined(parts)
            assert ranks.shape == (B, n, MAX_PREFIX + 3) and ranks.dtype == np.int32 and top_ids.shape == (B, n, TOP)
            assert np.array_equal(cnt, np.broadcast_to(np.minimum(np.arange(n), N), (B, n)))
            assert parts[-1].state.count == min(n, N) and parts[-1].state.pos == n
            # every cut of the stream: the same ranks and lists, bit for bit
            for cuts in (CUTS[0], CUTS[2]):
                r2, i2, l2, c2 = joined(run_cut(model, x, y, spec, cuts))
                assert np.array_equal(r2, ranks) and np.array_equal(i2, top_ids) and l2.tobytes() == top_logp.tobytes(), (name, N, theta, cuts)
            # step 0 of a fresh stream: the plain rank
            assert np.array_equal(ranks[:, 0], plain_before[:, 0])
            # the oracle's interval at delta_q
            scored = model.score_streams_cached(x, y, spec)
            assert torch.equal(parts[-1].state.hist.view(torch.int32), scored.state.hist.view(torch.int32))
            assert torch.equal(parts[-1].state.words, scored.state.words)
            assert torch.equal(parts[-1].h.view(torch.int32), scored.h.view(torch.int32)) and torch.equal(parts[-1].c, scored.c)
            nll_mix = scored.nll(LAM)
            kb_old = np.stack([position_bars(dev_h[b], dev_h[b], y[b], N, [theta], bool(m.split_lstm))[0] for b in range(B)])
            single = total = 0
            worst_bar = 0.0
            for b in range(B):
                c, wc = C.cache_distribution(ora_h[b], y[b], N, theta, m.V)
                assert np.array_equal(wc, cnt[b])
                ymix = C.mixed_logits(ora_y[b], c, LAM, sn)
                bars = mix_bars(dev_h[b], ora_h[b], y[b], ora_y[b], ymix, N, theta, LAM, bool(m.split_lstm), sn)
                kb_new = mix_bars(dev_h[b], dev_h[b], y[b], ora_y[b], ymix, N, theta, LAM, bool(m.split_lstm), sn)
                worst_bar = max(worst_bar, float(bars.max()))
                for q in range(n):
                    t = int(y[b, q])
                    delta = 2 * rc.DELTA + bars[q]
                    for col, S in enumerate(sets[t]):
                        if S is None:
                            assert ranks[b, q, col] == -1, (name, N, theta, b, q, col)
                            continue
                        lo, hi = rc.interval(ymix[q], t, S, delta)
                        total += 1
                        single += lo == hi
                        assert lo <= ranks[b, q, col] <= hi, (name, N, theta, b, q, col, int(ranks[b, q, col]), lo, hi, delta)
                    # column A < k <=> the target is among the first k of the list
                    for k in (1, 5, 10):
                        assert (ranks[b, q, 0] < k) == (t in top_ids[b, q, :k]), (name, N, theta, b, q, k)
                    # the list's log p of the target is the mixture score_streams_cached reports
                    at = np.flatnonzero(top_ids[b, q] == t)
                    if len(at):
                        err = abs(top_logp[b, q, at[0]] + nll_mix[b, q])
                        assert err <= TOK_ATOL + kb_old[b, q] + kb_new[q], (name, N, theta, b, q, err)
                assert np.all(np.diff(top_logp[b], axis=1) <= 0)           # most probable first
            print("%s N %d theta %.1f: %d / %d (token, level) intervals are a single rank; largest cache bar %.3e" %
                  (name, N, theta, single, total, worst_bar))
            # the cache moves ranks on a stream over a dozen words, and repeated words rise
            rep = np.zeros((B, n), dtype=bool)
            for b in range(B):
                for q in range(1, n):
                    rep[b, q] = y[b, q] in y[b, max(q - N, 0):q]
            assert np.any(ranks[:, :, 0] != plain_before[:, :, 0])
            assert ranks[:, :, 0][rep].mean() < plain_before[:, :, 0][rep].mean()
    # lam = 0: rank_streams' array
    zero = model.rank_streams_cached(x, y, C.CacheSpec(16, theta=0.5, lam=0.0), max_prefix=MAX_PREFIX)
    assert np.array_equal(zero.ranks, plain_before) and zero.top_ids is None
    # rank_streams is what it was
    assert np.array_equal(model.rank_streams(x, y, max_prefix=MAX_PREFIX)[0], plain_before)


@pytest.mark.parametrize("name", MODELS)
def test_predict_next_cached_is_the_loops_step(name, fx, monkeypatch):
    """The one-step form against the loop: a call of k steps, then a call of ONE step with lists.  That step's list is formed from
    the state the step wrote (the second call's h) and the cache as it stood before the step's own write (the first call's state):
    predict_next_cached over those two gives the same ids and log p, and with ``allowed`` the position of a word in the restricted
    list is its prefix-level rank."""
    f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    index = model.reading_index()
    x, y = _stream(m.V, seed=12)
    spec = C.CacheSpec(16, theta=0.5, lam=LAM)
    k = 30
    first = model.rank_streams_cached(x[:, :k], y[:, :k], spec, max_prefix=MAX_PREFIX)
    step = model.rank_streams_cached(x[:, k:k + 1], y[:, k:k + 1], spec, first.h, first.c, first.state, max_prefix=MAX_PREFIX, top=TOP)
    got = model.predict_next_cached(step.h, first.state, spec, n=TOP)
    for b in range(x.shape[0]):
        assert np.array_equal(got[b][0], step.top_ids[b, 0]) and got[b][1].tobytes() == step.top_logp[b, 0].tobytes(), (name, b)
    # restricted to the words whose reading starts with the target's first kana: the target's position is its level-1 rank
    allowed, want = [], []
    for b in range(x.shape[0]):
        t = int(y[b, k])
        S = rc.level_sets(index, t, MAX_PREFIX)[2]
        allowed.append(None if S is None else S)
        want.append(int(step.ranks[b, 0, 0 if S is None else 2]))
    lists = model.predict_next_cached(step.h, first.state, spec, n=64, allowed=allowed)
    for b in range(x.shape[0]):
        ids = lists[b][0]
        at = np.flatnonzero(ids == int(y[b, k]))
        assert (want[b] < len(ids)) == bool(len(at)) and (not len(at) or int(at[0]) == want[b]), (name, b, want[b], ids[:5])
        if allowed[b] is not None:
            assert set(ids.tolist()) <= set(int(w) for w in allowed[b])
    # an empty cache: the model's own list
    plain = model.predict_next_cached(step.h, None, spec, n=5)
    none = model.predict_next_cached(step.h, first.state, C.CacheSpec(16, theta=0.5, lam=0.0), n=5)
    for b in range(x.shape[0]):
        assert np.array_equal(plain[b][0], none[b][0]) and plain[b][1].tobytes() == none[b][1].tobytes()


@pytest.mark.parametrize("name", ["small-tied", "small-tied-sn"])
def test_rank_cached_ragged_sequences(name, fx, monkeypatch):
    """ragged sequences, empty ones included, each from an empty cache, in rank()'s row plan: every sequence ranks as its own stream"""
    _f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    rng = np.random.RandomState(2)
    pool = rng.randint(2, m.V, size=6)
    seqs = [[int(w) for w in pool[rng.randint(0, 6, size=L)]] for L in (9, 0, 30, 1, 17, 0, 30)]
    spec = C.CacheSpec(8, theta=0.7, lam=0.25)
    got = model.rank_cached(seqs, 1, spec, max_prefix=MAX_PREFIX)
    cut = model.rank_cached(seqs, 1, spec, max_prefix=MAX_PREFIX, max_rows=2)
    plain = model.rank(seqs, 1, max_prefix=MAX_PREFIX)
    assert [g.shape for g in got] == [(len(s), MAX_PREFIX + 3) for s in seqs]
    moved = 0
    for s, g, g2, p in zip(seqs, got, cut, plain):
        assert np.array_equal(g, g2)
        if not len(s):
            continue
        one = model.rank_streams_cached(np.array([[1] + s[:-1]]), np.array([s]), spec, max_prefix=MAX_PREFIX)
        assert np.array_equal(one.ranks[0], g)
        assert np.array_equal(g[0], p[0])                                  # an empty cache: the plain rank
        moved += int(np.any(g != p))
    assert moved


def test_perplexity_command_line_ranks_with_cache(fx, tmp_path, capsys):
    """--ranks --cache prints a second --ranks line "with cache" over the same tokens, equal to the metrics of rank_streams_cached over
    the same chunks; without --cache the --ranks output is what it was"""
    from jlm_amd import config as jconfig, perplexity, rank as R
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
    args = ["--root", f["root"], "-e", "1", "--mode", "stream", "-b", "4", "--num_steps", "5", "--file", path, "--ranks"]
    perplexity.main(args)
    plain = [ln for ln in capsys.readouterr().out.splitlines() if "top-1:" in ln]
    perplexity.main(args + ["--cache", "40", "--theta", "0.5", "--lam", "0.2"])
    out = [ln for ln in capsys.readouterr().out.splitlines() if "top-1:" in ln]
    assert len(plain) == 1 and len(out) == 2 and out[0] == plain[0] and out[1].startswith("with cache (N 40 theta 0.5 lam 0.2): ")
    model = load_model(f["root"])
    sents, _unk = perplexity.encode_lines(perplexity.read_lines(path), vocab)
    x, y = stream_layout([i for s in sents for i in s], 4, 5)
    spec = C.CacheSpec(40, 0.5, 0.2)
    h = c = state = None
    parts = []
    for i in range(x.shape[1] // 5):
        res = model.rank_streams_cached(x[:, 5 * i:5 * i + 5], y[:, 5 * i:5 * i + 5], spec, h, c, state)
        h, c, state = res.h, res.c, res.state
        parts.append(res.ranks)
    ranks = np.concatenate(parts, axis=1)
    want = perplexity.ranks_line(ranks.reshape(-1, ranks.shape[-1]), y.reshape(-1).astype(np.int64), model.reading_index(), [1, 5, 10], 5)
    assert out[1] == "with cache (N 40 theta 0.5 lam 0.2): " + want
    mrr = lambda line: float(line.split("MRR: ")[1].split()[0])
    assert mrr(out[1]) > mrr(out[0])                                       # a repeated passage: the cache lifts the words it has seen
    assert R.mrr(ranks) == pytest.approx(mrr(out[1]), abs=1e-4)


def test_refusals(fx, monkeypatch):
    _f, model = fixture_model(fx, "small-tied", monkeypatch)
    _f2, other = fixture_model(fx, "small-vtable", monkeypatch)
    x, y = _stream(model.dev.V, n=6)
    spec = C.CacheSpec(4)
    res = model.rank_streams_cached(x, y, spec, readings=False)
    with pytest.raises(ValueError, match="one theta"):
        model.rank_streams_cached(x, y, C.CacheSpec(4, theta=[0.1, 0.2]), readings=False)
    with pytest.raises(ValueError, match="at most 4096"):
        model.rank_streams_cached(x, y, C.CacheSpec(4097), readings=False)
    with pytest.raises(ValueError, match="another model"):
        other.rank_streams_cached(x, y, spec, state=res.state, readings=False)
    with pytest.raises(ValueError, match="streams"):
        model.rank_streams_cached(x[:2], y[:2], spec, state=res.state, readings=False)
    with pytest.raises(ValueError, match="top"):
        model.rank_streams_cached(x, y, spec, readings=False, top=65)
    with pytest.raises(ValueError, match="another model"):
        other.predict_next_cached(res.h, res.state, spec)
    # a state of score_streams_cached continues a ranking call, and the other way round
    sc = model.score_streams_cached(x, y, spec)
    a = model.rank_streams_cached(x, y, spec, sc.h, sc.c, sc.state, readings=False)
    b = model.rank_streams_cached(x, y, spec, res.h, res.c, res.state, readings=False)
    assert np.array_equal(a.ranks, b.ranks)
    model.score_streams_cached(x, y, spec, res.h, res.c, res.state)


def test_untied_split_model_has_no_one_step_form(fx, monkeypatch):
    _f, model = fixture_model(fx, "small-untied", monkeypatch)
    assert model.dev.split_lstm and model.dev.mode == "untied"
    x, y = _stream(model.dev.V, n=4)
    res = model.rank_streams_cached(x, y, C.CacheSpec(4), readings=False)
    with pytest.raises(ValueError, match="untied split-row"):
        model.predict_next_cached(res.h, res.state, C.CacheSpec(4))
