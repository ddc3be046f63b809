"""CPU: ranking and prediction under the continuous cache (LSTM_Model.rank_streams_cached / rank_cached / predict_next_cached,
jlm_amd/cache.py) -- the float64 definition against itself and against cache_log_probs, the host path end to end
over the numpy double of the new entry points (tests/fake_cache_mix.py) on the models of tests/rank_cases.py, every refusal, and the
condition that keeps the GPU comparison (tests/test_gpu_rank_cache.py) from being vacuous."""
import numpy as np
import pytest

from jlm_amd import cache as C
from tests import context_cases as cc
from tests import fake_cache_mix
from tests import rank_cases as rc
from tests.cache_mix_budget import lpc_bar, lse_bar, y_bar

LAM = 0.2
MAX_PREFIX = 3
CUTS = ([45], [20, 20, 5], [7, 38])


@pytest.fixture()
def fake(monkeypatch):
    return fake_cache_mix.install(monkeypatch)


def _model(name):
    cc.set_root(name)
    from jlm_amd.model import LSTM_Model
    return LSTM_Model(experiment_id=1)


def _stream(V, B=3, n=45, seed=11):
    """B streams of n steps over a pool of a dozen words (tests/test_gpu_cache.py _stream): matches and misses both occur"""
    rng = np.random.RandomState(seed)
    pool = rng.randint(2, V, size=12)
    s = pool[rng.randint(0, 12, size=(B, n + 1))].astype(np.int32)
    return s[:, :-1], s[:, 1:]


def _lse(y):
    m = y.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(y - m).sum(axis=-1, keepdims=True)))[..., 0]


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("size, theta", [(1, 0.7), (4, 0.0), (7, 2.0), (50, 0.3)])
def test_cache_distribution_sums_to_one_and_agrees_with_cache_log_probs(size, theta):
    rng = np.random.RandomState(size)
    n, H, V = 30, 32, 9
    h = rng.uniform(-0.6, 0.6, size=(n, H))
    w = rng.randint(0, 6, size=n)                                           # words 6 .. 8 never occur
    c, cnt = C.cache_distribution(h, w, size, theta, V)
    lpc, cnt2 = C.cache_log_probs(h, w, size, [theta])
    assert c.shape == (n, V) and np.array_equal(cnt, cnt2) and np.array_equal(cnt, np.minimum(np.arange(n), size))
    assert np.all(c[0] == 0) and np.allclose(c[1:].sum(axis=1), 1.0, rtol=0, atol=1e-12) and np.all(c[:, 6:] == 0)
    with np.errstate(divide="ignore"):
        got = np.log(c[np.arange(n), w])
    assert np.array_equal(np.isneginf(got), np.isneginf(lpc[0]))
    ok = np.isfinite(got)
    assert np.allclose(got[ok], lpc[0][ok], rtol=0, atol=1e-12)
    for q in range(1, n):                                                   # mass only on the words of the window
        assert set(np.flatnonzero(c[q])) == set(w[max(q - size, 0):q])
    # the entries carried into a call: the same rows
    c2, cnt3 = C.cache_distribution(h, w, size, theta, V, carried=11)
    assert np.array_equal(c2, c[11:]) and np.array_equal(cnt3, cnt[11:])
    with pytest.raises(ValueError):
        C.cache_distribution(h, w, size, theta, 5)


@pytest.mark.parametrize("self_norm", [False, True])
def test_mixed_logits_order_as_the_mixture(self_norm):
    rng = np.random.RandomState(3)
    V = 40
    y = 2.0 * rng.standard_normal((6, V))
    if self_norm:
        y -= _lse(y)[:, None] + 0.05 * rng.standard_normal((6, 1))         # about normalised, as such a model's logits are
    c = np.zeros((6, V))
    for r in range(1, 6):
        at = rng.choice(V, size=r + 1, replace=False)
        c[r, at] = rng.dirichlet(np.ones(r + 1))
    y[2, np.flatnonzero(c[2])[0]] = -np.inf                                 # a cached word the model gives no mass
    L = np.zeros(6) if self_norm else _lse(y)
    p = (1 - LAM) * np.exp(y - L[:, None]) + LAM * c
    p[0] = np.exp(y[0] - L[0])                                              # an empty window: the model's own distribution
    got = C.mixed_logits(y, c, LAM, self_norm)
    assert got[0].tobytes() == y[0].tobytes() and np.all(got[c == 0] == y[c == 0])
    for r in range(6):
        assert np.array_equal(np.lexsort((np.arange(V), -got[r])), np.lexsort((np.arange(V), -p[r]))), r
    if not self_norm:                                                       # (self_norm: L = 0 by definition, whatever lse(y) is)
        assert np.allclose(_lse(got[1:]), L[1:] - np.log1p(-LAM), rtol=0, atol=1e-12)
    assert np.allclose(got[1:] - (L[1:] - np.log1p(-LAM))[:, None], np.log(p[1:]), rtol=0, atol=1e-12)
    assert np.isfinite(got[2]).all() and C.mixed_logits(y, c, 0.0, self_norm).tobytes() == y.tobytes()
    with pytest.raises(ValueError):
        C.mixed_logits(y, c[:, :-1], LAM)
    with pytest.raises(ValueError):
        C.mixed_logits(y, c, 1.0)


# ---------------------------------------------------------------------------------------------- the host path over the double
def _run_cut(m, x, y, spec, cuts, top=5):
    h = c = state = None
    parts, at = [], 0
    for k in cuts:
        res = m.rank_streams_cached(x[:, at:at + k], y[:, at:at + k], spec, h, c, state, max_prefix=MAX_PREFIX, top=top)
        h, c, state = res.h, res.c, res.state
        parts.append(res)
        at += k
    return (np.concatenate([p.ranks for p in parts], axis=1), np.concatenate([p.top_ids for p in parts], axis=1),
            np.concatenate([p.top_logp for p in parts], axis=1), parts[-1])


def _oracle_mixed(name, x, y, N, theta):
    """-> (ymix [B, n, V] float64: mixed_logits over the oracle's logits with cache_distribution over its states, h [B, n, H], y)"""
    lm = cc.oracle(name).model
    B, n = x.shape
    h, c = lm.zero_state(B)
    hs, ys = [], []
    for t in range(n):
        h, c = lm.lstm_cell(x[:, t], h, c)
        ys.append(np.array(lm.project(h), dtype=np.float64))
        hs.append(np.array(h, dtype=np.float64))
    hs, ys = np.stack(hs, axis=1), np.stack(ys, axis=1)
    sn = bool(lm.config["self_norm"])
    out = np.stack([C.mixed_logits(ys[b], C.cache_distribution(hs[b], y[b], N, theta, ys.shape[2])[0], LAM, sn) for b in range(B)])
    return out, hs, ys, sn


@pytest.mark.parametrize("name", rc.MODELS)
def test_rank_streams_cached_end_to_end(name, fake):
    import torch
    m = _model(name)
    V = cc.MODELS[name][0]
    x, y = _stream(V)
    B, n = x.shape
    plain = m.rank_streams(x, y, max_prefix=MAX_PREFIX)[0]
    zero = m.rank_streams_cached(x, y, C.CacheSpec(16, theta=0.5, lam=0.0), max_prefix=MAX_PREFIX)
    assert np.array_equal(zero.ranks, plain) and zero.top_ids is None and zero.top_logp is None      # lam = 0: rank_streams' array
    N, theta = 16, 0.5
    spec = C.CacheSpec(N, theta=theta, lam=LAM)
    ranks, ids, logp, last = _run_cut(m, x, y, spec, CUTS[1])
    assert ranks.shape == plain.shape and ranks.dtype == np.int32 and ids.shape == logp.shape == (B, n, 5)
    assert np.array_equal(ranks[:, 0], plain[:, 0])                         # step 0 of a fresh stream: the plain rank
    for cuts in (CUTS[0], CUTS[2]):
        r2, i2, l2, _ = _run_cut(m, x, y, spec, cuts)
        assert np.array_equal(r2, ranks) and np.array_equal(i2, ids) and l2.tobytes() == logp.tobytes(), cuts
    # inside the oracle's interval; the list agrees with column A; log p of a listed target is the scored mixture.  delta = 2 DELTA
    # (the logit and L, tests/test_gpu_rank_cache.py) + DELTA for the cache term: the double sums in float64 over the double's own
    # states, which are within the f32 rounding of a step of the oracle's -- theta |D| H of a score, far below DELTA.  The log p
    # bar: tests/test_gpu_score.py's TOK_ATOL = 1e-5, once for the list's normaliser and once for the scored nll.
    ymix, _hs, _ys, sn = _oracle_mixed(name, x, y, N, theta)
    index = m.reading_index()
    sets = {int(t): rc.level_sets(index, int(t), MAX_PREFIX) for t in np.unique(y)}
    scored = m.score_streams_cached(x, y, spec)
    nll = scored.nll(LAM)
    for b in range(B):
        for q in range(n):
            t = int(y[b, q])
            for col, S in enumerate(sets[t]):
                if S is None:
                    assert ranks[b, q, col] == -1
                    continue
                lo, hi = rc.interval(ymix[b, q], t, S, 3 * rc.DELTA)
                assert lo <= ranks[b, q, col] <= hi, (name, b, q, col, int(ranks[b, q, col]), lo, hi)
            for k in (1, 5):
                assert (ranks[b, q, 0] < k) == (t in ids[b, q, :k])
            at = np.flatnonzero(ids[b, q] == t)
            if len(at):
                assert abs(logp[b, q, at[0]] + nll[b, q]) <= 2e-5, (name, b, q)
    # the rings hold what score_streams_cached puts there, and the carried state is its state
    bits = lambda t: t.view(torch.int32).numpy()
    assert np.array_equal(bits(last.state.hist), bits(scored.state.hist)) and np.array_equal(last.state.words.numpy(), scored.state.words.numpy())
    assert np.array_equal(bits(last.h), bits(scored.h)) and np.array_equal(bits(last.c), bits(scored.c)) and last.state.pos == scored.state.pos == n
    # the cache moves ranks, and repeated words rise
    rep = np.array([[q > 0 and y[b, q] in y[b, max(q - N, 0):q] for q in range(n)] for b in range(B)])
    assert np.any(ranks[:, :, 0] != plain[:, :, 0]) and ranks[:, :, 0][rep].mean() < plain[:, :, 0][rep].mean()
    assert np.array_equal(m.rank_streams(x, y, max_prefix=MAX_PREFIX)[0], plain)                     # rank_streams is what it was


@pytest.mark.parametrize("name", ["tied", "vtable"])
def test_predict_next_cached_is_the_loops_step(name, fake):
    """tests/test_gpu_rank_cache.py's check of the one-step form, over the double"""
    m = _model(name)
    V = cc.MODELS[name][0]
    index = m.reading_index()
    x, y = _stream(V, seed=12)
    spec = C.CacheSpec(16, theta=0.5, lam=LAM)
    k = 30
    first = m.rank_streams_cached(x[:, :k], y[:, :k], spec, max_prefix=MAX_PREFIX)
    step = m.rank_streams_cached(x[:, k:k + 1], y[:, k:k + 1], spec, first.h, first.c, first.state, max_prefix=MAX_PREFIX, top=10)
    got = m.predict_next_cached(step.h, first.state, spec, n=10)
    allowed, want = [], []
    for b in range(x.shape[0]):
        assert np.array_equal(got[b][0], step.top_ids[b, 0]) and got[b][1].tobytes() == step.top_logp[b, 0].tobytes()
        S = rc.level_sets(index, int(y[b, k]), MAX_PREFIX)[2]
        allowed.append(S)
        want.append(int(step.ranks[b, 0, 0 if S is None else 2]))
    lists = m.predict_next_cached(step.h, first.state, spec, n=min(64, V), allowed=allowed)
    for b in range(x.shape[0]):
        at = np.flatnonzero(lists[b][0] == int(y[b, k]))
        assert (want[b] < len(lists[b][0])) == bool(len(at)) and (not len(at) or int(at[0]) == want[b])
    assert [len(i) for i, _ in m.predict_next_cached(step.h, first.state, spec, n=3, allowed=[[], None, [2, 3]])] == [0, 3, 2]


def test_rank_cached_ragged_sequences(fake):
    m = _model("tied")
    V = cc.MODELS["tied"][0]
    rng = np.random.RandomState(2)
    pool = rng.randint(2, V, size=6)
    seqs = [[int(w) for w in pool[rng.randint(0, 6, size=L)]] for L in (9, 0, 30, 1, 17, 0, 30)]
    spec = C.CacheSpec(8, theta=0.7, lam=0.25)
    got = m.rank_cached(seqs, cc.EOS, spec, max_prefix=MAX_PREFIX)
    cut = m.rank_cached(seqs, cc.EOS, spec, max_prefix=MAX_PREFIX, max_rows=2)
    plain = m.rank(seqs, cc.EOS, max_prefix=MAX_PREFIX)
    assert [g.shape for g in got] == [(len(s), MAX_PREFIX + 3) for s in seqs]
    for s, g, g2, p in zip(seqs, got, cut, plain):
        assert np.array_equal(g, g2)
        if len(s):
            one = m.rank_streams_cached(np.array([[cc.EOS] + s[:-1]]), np.array([s]), spec, max_prefix=MAX_PREFIX)
            assert np.array_equal(one.ranks[0], g) and np.array_equal(g[0], p[0])
    assert any(np.any(g != p) for g, p in zip(got, plain))


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(fake):
    import torch
    m = _model("tied")
    other = _model("vtable")
    V = cc.MODELS["tied"][0]
    x, y = _stream(V, n=6)
    spec = C.CacheSpec(4)
    res = m.rank_streams_cached(x, y, spec, readings=False)
    del fake.launches[:]
    bad_specs = [C.CacheSpec(4, theta=[0.1, 0.2]), C.CacheSpec(4097), "spec", None]
    for s in bad_specs:
        with pytest.raises(ValueError):
            m.rank_streams_cached(x, y, s, readings=False)
        with pytest.raises(ValueError):
            m.rank_cached([[2, 3]], cc.EOS, s, readings=False)
        with pytest.raises(ValueError):
            m.predict_next_cached(res.h, res.state, s)
    for a, kw in (((x, y[:, :2]), {}), ((x[0], y[0]), {}), ((x, y), dict(h=res.h)), ((x, np.full_like(y, V)), {}), ((x, y), dict(top=65)),
                  ((x, y), dict(top=-1)), ((x, y), dict(top=1.5)), ((x, y), dict(max_prefix=40, readings=True)),
                  ((x[:2], y[:2]), dict(state=res.state)), ((x, y), dict(state="state")),
                  ((x, y), dict(h=torch.zeros(2, m.dev.H), c=torch.zeros(2, m.dev.H)))):
        args = dict(readings=False)
        args.update(kw)
        with pytest.raises(ValueError):
            m.rank_streams_cached(*a, spec, **args)
    with pytest.raises(ValueError, match="another model"):
        other.rank_streams_cached(x, y, spec, state=res.state, readings=False)
    with pytest.raises(ValueError, match="another model"):
        other.predict_next_cached(res.h, res.state, spec)
    for kw in (dict(n=0), dict(n=65), dict(allowed=[None]), dict(allowed=[[V], None, None])):
        with pytest.raises(ValueError):
            m.predict_next_cached(res.h, res.state, spec, **kw)
    with pytest.raises(ValueError):
        m.predict_next_cached(None, res.state, spec)
    with pytest.raises(ValueError):
        m.predict_next_cached(res.h[:2], res.state, spec)
    with pytest.raises(ValueError):
        m.rank_cached([[2, V]], cc.EOS, spec)
    assert fake.launches == []
    empty = m.rank_streams_cached(x[:, :0], y[:, :0], spec, state=res.state, top=3)
    assert empty.ranks.shape == (3, 0, rc.MAX_PREFIX + 3) and empty.state is res.state and empty.top_ids.shape == (3, 0, 3)
    assert m.rank_cached([], cc.EOS, spec) == [] and fake.launches == []


def test_untied_split_model_has_no_one_step_form(fake):
    m = _model("untied")
    assert m.dev.split_lstm
    x, y = _stream(cc.MODELS["untied"][0], n=4)
    res = m.rank_streams_cached(x, y, C.CacheSpec(4), readings=False)
    del fake.launches[:]
    with pytest.raises(ValueError, match="untied split-row"):
        m.predict_next_cached(res.h, res.state, C.CacheSpec(4))
    assert fake.launches == []


def test_double_refuses_what_the_header_refuses(fake):
    """the launchers' -1 cases through the double, as tests/test_gpu_cache_mix_rows.py asks them of the library"""
    hist = np.zeros((8, 2, 32), dtype=np.float32)
    q = np.zeros((2, 32), dtype=np.float32)
    words = np.zeros((8, 2), dtype=np.int32)
    first = np.zeros(2, dtype=np.int32)
    s = np.full((2, 8), 7.0, dtype=np.float32)
    y = np.zeros((2, 8), dtype=np.float32)
    a = lambda v: v.ctypes.data
    base_q = dict(hist=a(hist), cap=8, n_rows=2, H=32, split=0, h_scale=1.0, q_rows=a(q), n_rows_max=2, n_dev=None, pos=5, first=a(first), N=8,
                  theta=0.5, s=a(s), ld_s=8, flags=None, stream=None)
    base_m = dict(y=a(y), ld_y=8, n_cols=6, self_norm=0, s=a(s), ld_s=8, words=a(words), cap=8, n_rows=2, n_rows_max=2, n_dev=None, pos=5,
                  first=a(first), N=8, lam=0.2, lpc_ent=None, flags=None, stream=None)
    for kw in (dict(N=0), dict(N=4097, ld_s=4097, cap=4097), dict(cap=7), dict(ld_s=7), dict(H=48), dict(theta=-1.0), dict(theta=float("nan")),
               dict(pos=-1), dict(n_rows_max=3), dict(hist=None), dict(s=None), dict(first=None), dict(split=1, h_scale=0.0)):
        assert fake.jlm_cache_query(**dict(base_q, **kw)) == -1, kw
    for kw in (dict(N=0), dict(cap=7), dict(ld_s=7), dict(lam=-0.1), dict(lam=1.0), dict(n_cols=0), dict(ld_y=6), dict(y=None),
               dict(words=None), dict(n_rows_max=3)):
        assert fake.jlm_cache_mix_rows(**dict(base_m, **kw)) == -1, kw
    assert fake.launches == [] and fake.jlm_cache_mix_rows(**dict(base_m, lam=0.0)) == 0 and fake.launches == []
    assert np.all(s == 7.0) and not y.any()


# ---------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("name", rc.MODELS)
def test_oracle_interval_is_mostly_one_rank(name):
    """the non-vacuity condition of tests/test_gpu_rank_cache.py: at delta_q = 2 DELTA + the position's cache bar (here the kernels'
    derived bar over the oracle's own states: the device's states are not to hand, and their part of the bar is of the same order)
    the oracle's interval is a single rank for at least 80 % of the (token, level) entries of every model"""
    V = cc.MODELS[name][0]
    x, y = _stream(V)
    B, n = x.shape
    N, theta = 16, 2.0
    ymix, hs, ys, sn = _oracle_mixed(name, x, y, N, theta)
    from tests import predict_cases as pc
    index = pc.index_of(name)
    sets = {int(t): rc.level_sets(index, int(t), MAX_PREFIX) for t in np.unique(y)}
    log_rho = np.log(LAM) - np.log1p(-LAM)
    total = one = 0
    for b in range(B):
        for q in range(n):
            bar = 0.0
            lo_q = max(q - N, 0)
            if q > lo_q:
                k, ww = hs[b, lo_q:q], y[b, lo_q:q]
                A = float((np.abs(k) @ np.abs(hs[b, q])).max())
                sc = theta * (k @ hs[b, q])
                e = np.exp(sc - sc.max())
                logZ = np.log(e.sum())
                L = 0.0 if sn else float(_lse(ys[b, q]))
                for w in np.unique(ww):
                    logc = np.log(e[ww == w].sum())
                    bar = max(bar, y_bar(lpc_bar(True, hs.shape[2], N, theta, A, logc, logZ), lse_bar(ys[b, q], sn), L, log_rho, logc - logZ,
                                         ys[b, q, w], ymix[b, q, w]))
            t = int(y[b, q])
            for S in sets[t]:
                if S is not None:
                    lo, hi = rc.interval(ymix[b, q], t, S, 2 * rc.DELTA + bar)
                    assert hi >= lo
                    total += 1
                    one += lo == hi
    assert total >= 300 and one >= 0.8 * total, (name, one, total)
