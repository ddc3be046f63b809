"""GPU: ranking and prediction under a memory end to end (LSTM_Model.rank_streams_memory / rank_memory / predict_next_memory,
Memory.search; csrc jlm_rank_memory_frames, jlm_predict_memory_rows, jlm_memory_topk, cache_mix_rows_kernel) against the float64
definition: jlm_amd.cache.mixed_logits over the oracle's logits (OracleLM.project) with the memory's distribution over the oracle's own
states (OracleLM.lstm_cell), on the five models of tests/test_gpu_cache.py.  Streams of B = 3, n = 45; a memory of 135 entries built
from another text, as tests/test_gpu_memory.py builds it; theta 0.5 / 2.0, lam 0.2, K = 16 and K = 1024 (>= N).

Every device rank must lie in the interval the oracle's mixed logits leave open (tests/rank_cases.py interval) at

    delta_q = 2 * rank_cases.DELTA + the position's bar

as tests/test_gpu_rank_cache.py takes it; the bar is tests/cache_mix_budget.py's Y_BAR with the retrieval's product term
(tests/memory_topk_budget.py lpc_bar), maximised over the retrieved words, plus what the difference D between the device's states and
the oracle's can move a score, theta (|Dq . k| + |q . Dk| + |Dq . Dk|), maximised over the retrieved entries.  For K = 16 the
reference's c is taken over the neighbours the call returned -- tests/test_gpu_memory_topk.py establishes that they are a valid top-K
set of the device's scores --; for K >= N it is the pure definition, jlm_amd.memory.memory_distribution over the oracle's states."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import cache as C, memory as M                                                 # noqa: E402
from tests import rank_cases as rc                                                          # noqa: E402
from tests.cache_mix_budget import lse_bar, y_bar                                           # noqa: E402
from tests.gpu_rows import fixture_model, lse, oracle_lm                                    # noqa: E402
from tests.memory_topk_budget import lpc_bar                                                # noqa: E402
from tests.test_gpu_cache import MODELS, TOK_ATOL, oracle_states                            # noqa: E402
from tests.test_gpu_memory import _streams, bars as memory_bars, tb                         # noqa: E402
from tests.test_gpu_rank_cache import oracle_run                                            # noqa: E402

pytestmark = pytest.mark.gpu

LAM = 0.2
THETAS = [0.5, 2.0]
KS = [16, 1024]
CUTS = ([45], [20, 20, 5], [7, 38])
MAX_PREFIX = 3
TOP = 10


def distribution(q, keys, words, idx, theta, V):
    """c of the definition over the entries ``idx``, float64 -> (c [V], e [len(idx)] under the maximum)"""
    s = theta * (keys[idx] @ q)
    e = np.exp(s - s.max())
    c = np.zeros(V)
    np.add.at(c, words[idx], e)
    return c / e.sum(), e


def mix_bar(dev_q, ora_q, dev_k, ora_k, k_words, idx, e, ys, ymix, theta, lam, split, self_norm):
    """the bar of ONE position (module docstring)"""
    H = len(ora_q)
    k, dk, ww, D = ora_k[idx], dev_k[idx] - ora_k[idx], k_words[idx], dev_q - ora_q
    move = float((np.abs(k @ D) + np.abs(dk @ ora_q) + np.abs(dk @ D)).max())
    A = float((np.abs(dev_k[idx]) @ np.abs(dev_q)).max())
    log_rho = np.log(lam) - np.log1p(-lam)
    logZ = np.log(e.sum())
    L = 0.0 if self_norm else float(lse(ys))
    L_b = lse_bar(ys, self_norm)
    out = 0.0
    for w in np.unique(ww):
        logc = np.log(e[ww == w].sum())
        b = lpc_bar(split, H, len(idx), theta, A, logc, logZ) + theta * move
        out = max(out, y_bar(b, L_b, L, log_rho, logc - logZ, ys[w], ymix[w]))
    return out


def run_cut(model, x, y, mix, cuts, top=TOP):
    h = c = None
    parts, at = [], 0
    for k in cuts:
        res = model.rank_streams_memory(x[:, at:at + k], y[:, at:at + k], mix, h, c, max_prefix=MAX_PREFIX, top=top, neighbours=True)
        h, c = res.h, res.c
        parts.append(res)
        at += k
    return parts


def joined(parts):
    return (np.concatenate([p.ranks for p in parts], axis=1), np.concatenate([p.top_ids for p in parts], axis=1),
            np.concatenate([p.top_logp for p in parts], axis=1), np.concatenate([p.neighbours for p in parts], axis=1))


@pytest.mark.parametrize("name", MODELS)
def test_streams_rank_inside_the_oracles_interval(name, fx, monkeypatch):
    f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    lm = oracle_lm(f["root"])
    index = model.reading_index()
    (xm, ym), (x, y) = _streams(m.V)
    B, n = x.shape
    sn, split = bool(m.self_norm), bool(m.split_lstm)
    ora_k = tb(oracle_states(lm, xm, ym)[0])
    k_words = tb(ym).astype(np.int64)
    ora_h, ora_y = oracle_run(lm, x)
    memory = M.Memory.build(model, xm, ym, 20)
    N = memory.N
    assert N == B * n == 135
    dev_k = memory.numpy()[0].astype(np.float64)
    queries = M.Memory.build(model, x, y, n)                                           # the device's own query states, order (t, b)
    dev_q = queries.numpy()[0].astype(np.float64).reshape(n, B, -1)
    plain_before, h_plain, c_plain = model.rank_streams(x, y, max_prefix=MAX_PREFIX)
    sets = {int(t): rc.level_sets(index, int(t), MAX_PREFIX) for t in np.unique(y)}
    present = np.isin(y, ym)
    assert present.any() and not present.all()
    for K in KS:
        n_q = min(K, N)
        for theta in THETAS:
            mix = M.MemoryMix(memory, theta=theta, lam=LAM, k=K)
            parts = run_cut(model, x, y, mix, CUTS[1])
            ranks, top_ids, top_logp, nb = joined(parts)
            assert ranks.shape == (B, n, MAX_PREFIX + 3) and ranks.dtype == np.int32 and top_ids.shape == (B, n, TOP)
            assert nb.shape == (B, n, n_q) and nb.dtype == np.int64 and nb.min() >= 0 and nb.max() < N
            assert all(len(set(nb[b, q].tolist())) == n_q for b in range(B) for q in range(n))
            # every cut of the stream: the same ranks, lists and neighbours, bit for bit; the state is rank_streams'
            for cuts in (CUTS[0], CUTS[2]):
                p2 = run_cut(model, x, y, mix, cuts)
                r2, i2, l2, n2 = joined(p2)
                assert np.array_equal(r2, ranks) and np.array_equal(i2, top_ids) and l2.tobytes() == top_logp.tobytes() and np.array_equal(n2, nb), \
                    (name, K, theta, cuts)
                assert torch.equal(p2[-1].h.view(torch.int32), h_plain.view(torch.int32)) and torch.equal(p2[-1].c, c_plain)
            # Memory.search over the same states: the same neighbours
            idx, sc, words = memory.search(queries.keys, K, theta)
            assert np.array_equal(idx.reshape(n, B, n_q).transpose(1, 0, 2), nb) and np.array_equal(words, k_words[idx])
            assert sc.dtype == np.float32 and np.all(np.diff(sc, axis=1) <= 0)
            if K >= N:
                scored = model.score_streams_memory(x, y, memory, M.MemorySpec(theta=theta, lam=LAM))
                nll_mix = scored.nll(LAM)
                kb_old = memory_bars(tb(dev_q.transpose(1, 0, 2)), tb(dev_q.transpose(1, 0, 2)), dev_k, dev_k, tb(y), k_words, [theta],
                                     split)[0].reshape(n, B)
            single = total = 0
            worst_bar = 0.0
            for b in range(B):
                for q in range(n):
                    if K >= N:
                        c = M.memory_distribution(ora_h[b, q], ora_k, k_words, theta, K, m.V)
                        sel = np.arange(N)
                        e = np.exp(theta * (ora_k @ ora_h[b, q]) - (theta * (ora_k @ ora_h[b, q])).max())
                        assert set(nb[b, q].tolist()) == set(range(N))
                    else:
                        sel = nb[b, q]
                        c, e = distribution(ora_h[b, q], ora_k, k_words, sel, theta, m.V)
                    ymix = C.mixed_logits(ora_y[b, q], c, LAM, sn)
                    bar = mix_bar(dev_q[q, b], ora_h[b, q], dev_k, ora_k, k_words, sel, e, ora_y[b, q], ymix, theta, LAM, split, sn)
                    worst_bar = max(worst_bar, bar)
                    t = int(y[b, q])
                    delta = 2 * rc.DELTA + bar
                    for col, S in enumerate(sets[t]):
                        if S is None:
                            assert ranks[b, q, col] == -1, (name, K, theta, b, q, col)
                            continue
                        lo, hi = rc.interval(ymix, t, S, delta)
                        total += 1
                        single += lo == hi
                        assert lo <= ranks[b, q, col] <= hi, (name, K, theta, b, q, col, int(ranks[b, q, col]), lo, hi, delta)
                    # column A < k <=> the target is among the first k of the list
                    for k in (1, 5, 10):
                        assert (ranks[b, q, 0] < k) == (t in top_ids[b, q, :k]), (name, K, theta, b, q, k)
                    # K >= N: the list's log p of the target is the mixture score_streams_memory reports
                    at = np.flatnonzero(top_ids[b, q] == t)
                    if K >= N and len(at):
                        kb_new = mix_bar(dev_q[q, b], dev_q[q, b], dev_k, dev_k, k_words, sel, e, ora_y[b, q], ymix, theta, LAM, split, sn)
                        err = abs(top_logp[b, q, at[0]] + nll_mix[b, q])
                        assert err <= TOK_ATOL + kb_old[q, b] + kb_new, (name, K, theta, b, q, err)
                assert np.all(np.diff(top_logp[b], axis=1) <= 0)           # most probable first
            print("%s K %d theta %.1f: %d / %d (token, level) intervals are a single rank; largest bar %.3e" %
                  (name, K, theta, single, total, worst_bar))
            # the memory's text shares nine of the stream's twelve words: those rise
            assert np.any(ranks[:, :, 0] != plain_before[:, :, 0])
            assert ranks[:, :, 0][present].mean() < plain_before[:, :, 0][present].mean()
    # lam = 0: rank_streams' array
    zero = model.rank_streams_memory(x, y, M.MemoryMix(memory, theta=0.5, lam=0.0, k=16), max_prefix=MAX_PREFIX)
    assert np.array_equal(zero.ranks, plain_before) and zero.top_ids is None and zero.neighbours is None
    # rank_streams is what it was
    assert np.array_equal(model.rank_streams(x, y, max_prefix=MAX_PREFIX)[0], plain_before)


@pytest.mark.parametrize("name", MODELS)
def test_predict_next_memory_is_the_loops_step(name, fx, monkeypatch):
    """The one-step form against the loop: a call of k steps, then a call of ONE step with lists.  That step's list is formed from the
    state the step wrote (the second call's h): predict_next_memory over it gives the same ids and log p, and with ``allowed`` the
    position of a word in the restricted list is its prefix-level rank."""
    _f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    index = model.reading_index()
    (xm, ym), (x, y) = _streams(m.V)
    memory = M.Memory.build(model, xm, ym, 20)
    k = 30
    for K in KS:
        mix = M.MemoryMix(memory, theta=0.5, lam=LAM, k=K)
        first = model.rank_streams_memory(x[:, :k], y[:, :k], mix, max_prefix=MAX_PREFIX)
        step = model.rank_streams_memory(x[:, k:k + 1], y[:, k:k + 1], mix, first.h, first.c, max_prefix=MAX_PREFIX, top=TOP)
        got = model.predict_next_memory(step.h, mix, n=TOP)
        for b in range(x.shape[0]):
            assert np.array_equal(got[b][0], step.top_ids[b, 0]) and got[b][1].tobytes() == step.top_logp[b, 0].tobytes(), (name, K, b)
        allowed, want = [], []
        for b in range(x.shape[0]):
            t = int(y[b, k])
            S = rc.level_sets(index, t, MAX_PREFIX)[2]
            allowed.append(None if S is None else S)
            want.append(int(step.ranks[b, 0, 0 if S is None else 2]))
        lists = model.predict_next_memory(step.h, mix, n=64, allowed=allowed)
        for b in range(x.shape[0]):
            ids = lists[b][0]
            at = np.flatnonzero(ids == int(y[b, k]))
            assert (want[b] < len(ids)) == bool(len(at)) and (not len(at) or int(at[0]) == want[b]), (name, K, b, want[b], ids[:5])
            if allowed[b] is not None:
                assert set(ids.tolist()) <= set(int(w) for w in allowed[b])
    # lam = 0: the model's own list
    plain = model.predict_next_cached(step.h, None, C.CacheSpec(16, theta=0.5, lam=LAM), n=5)
    none = model.predict_next_memory(step.h, M.MemoryMix(memory, theta=0.5, lam=0.0, k=16), n=5)
    for b in range(x.shape[0]):
        assert np.array_equal(plain[b][0], none[b][0]) and plain[b][1].tobytes() == none[b][1].tobytes()


@pytest.mark.parametrize("name", ["small-tied", "small-tied-sn"])
def test_rank_memory_ragged_sequences(name, fx, monkeypatch):
    """ragged sequences, empty ones included, in rank()'s row plan: every sequence ranks as its own stream"""
    _f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    (xm, ym), (_x, y) = _streams(m.V)
    memory = M.Memory.build(model, xm, ym, 20)
    seqs = [[int(w) for w in y[i % 3, :L]] for i, L in enumerate((9, 0, 30, 1, 17, 0, 30))]
    mix = M.MemoryMix(memory, theta=0.7, lam=0.25, k=16)
    got = model.rank_memory(seqs, 1, mix, max_prefix=MAX_PREFIX)
    cut = model.rank_memory(seqs, 1, mix, max_prefix=MAX_PREFIX, max_rows=2)
    plain = model.rank(seqs, 1, max_prefix=MAX_PREFIX)
    assert [g.shape for g in got] == [(len(s), MAX_PREFIX + 3) for s in seqs]
    moved = 0
    for s, g, g2, p in zip(seqs, got, cut, plain):
        assert np.array_equal(g, g2)
        if not len(s):
            continue
        one = model.rank_streams_memory(np.array([[1] + s[:-1]]), np.array([s]), mix, max_prefix=MAX_PREFIX)
        assert np.array_equal(one.ranks[0], g)
        moved += int(np.any(g != p))
    assert moved


def test_refusals(fx, monkeypatch):
    _f, model = fixture_model(fx, "small-tied", monkeypatch)
    _f2, other = fixture_model(fx, "small-vtable", monkeypatch)
    (xm, ym), (x, y) = _streams(model.dev.V, n=6)
    memory = M.Memory.build(model, xm, ym, 6)
    mix = M.MemoryMix(memory, k=4)
    res = model.rank_streams_memory(x, y, mix, readings=False, neighbours=True)
    assert res.neighbours.shape == (3, 6, 4) and res.top_ids is None
    for bad in (dict(k=0), dict(k=1025), dict(k=2.5), dict(theta=[0.1, 0.2]), dict(theta=-1.0), dict(lam=1.0)):
        with pytest.raises(ValueError):
            M.MemoryMix(memory, **bad)
    with pytest.raises(ValueError):
        M.MemoryMix(None)
    with pytest.raises(ValueError, match="of this model"):
        other.rank_streams_memory(x, y, mix, readings=False)
    with pytest.raises(ValueError, match="of this model"):
        other.predict_next_memory(res.h, mix)
    with pytest.raises(ValueError, match="MemoryMix"):
        model.rank_streams_memory(x, y, M.MemorySpec(), readings=False)
    with pytest.raises(ValueError, match="top"):
        model.rank_streams_memory(x, y, mix, readings=False, top=65)
    with pytest.raises(ValueError):
        memory.search(res.h, 0)
    with pytest.raises(ValueError):
        memory.search(res.h[:, :8], 4)
    idx, sc, words = memory.search(res.h, 1024)
    assert idx.shape == sc.shape == words.shape == (3, memory.N)


def test_untied_split_model_is_refused_by_the_one_step_form_only(fx, monkeypatch):
    _f, model = fixture_model(fx, "small-untied", monkeypatch)
    assert model.dev.split_lstm and model.dev.mode == "untied"
    (xm, ym), (x, y) = _streams(model.dev.V, n=4)
    memory = M.Memory.build(model, xm, ym, 4)
    mix = M.MemoryMix(memory, k=4)
    res = model.rank_streams_memory(x, y, mix, readings=False)
    with pytest.raises(ValueError, match="untied split-row"):
        model.predict_next_memory(res.h, mix)
