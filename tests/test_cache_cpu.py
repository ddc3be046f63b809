"""CPU: the continuous cache of teacher-forced scoring (jlm_amd/cache.py) -- the float64 reference against a
brute-force loop over an explicit probability vector, the count identities at theta = 0 on the window's edges, the host path end to
end over the numpy double of the new entry points (tests/fake_cache.py): cutting invariance, the mixture, every refusal before a
launch, the tuner, the command line, the exports."""
import ctypes
import os

import numpy as np
import pytest

from jlm_amd import _lib, cache as C
from tests import context_cases as cc
from tests import fake_cache


@pytest.fixture()
def fake(monkeypatch):
    return fake_cache.install(monkeypatch)


def _model(name):
    cc.set_root(name)
    from jlm_amd.model import LSTM_Model
    return LSTM_Model(experiment_id=1)


# ---------------------------------------------------------------------------------------------- the reference
def brute_force(h, words, V, N, theta, first=0):
    """per position q the explicit cache distribution over the V words of a tiny vocabulary: p[w] = sum over the window's entries that
    were followed by w of softmax(theta h_q . h_i)"""
    n = len(words)
    out = np.zeros((n, V))
    cnt = np.zeros(n, dtype=int)
    for q in range(n):
        window = [i for i in range(n) if max(q - N, first) <= i < q]
        cnt[q] = len(window)
        if not window:
            continue
        s = np.array([theta * float(np.dot(h[q], h[i])) for i in window])
        a = np.exp(s - s.max())
        a /= a.sum()
        for i, ai in zip(window, a):
            out[q, words[i]] += ai
    return out, cnt


@pytest.mark.parametrize("N", [1, 3, 7, 50])
@pytest.mark.parametrize("theta", [0.0, 0.4, 3.0])
def test_reference_against_explicit_probability_vector(N, theta):
    rng = np.random.RandomState(N)
    V, n, H = 5, 24, 8
    h = rng.uniform(-1, 1, size=(n, H))
    words = rng.randint(0, V, size=n)
    lpc, cnt = C.cache_log_probs(h, words, N, [theta])
    p, want_cnt = brute_force(h, words, V, N, theta)
    assert np.array_equal(cnt, want_cnt) and np.array_equal(cnt, np.minimum(np.arange(n), N))
    for q in range(n):
        if cnt[q]:
            assert abs(p[q].sum() - 1.0) <= 1e-12                       # a probability vector
            np.testing.assert_allclose(np.exp(lpc[0, q]), p[q, words[q]], rtol=0, atol=1e-12)
            assert (lpc[0, q] == -np.inf) == (p[q, words[q]] == 0.0)
        else:
            assert lpc[0, q] == -np.inf and p[q].sum() == 0.0
    # carried entries: the same numbers for the positions behind them
    part, pc = C.cache_log_probs(h, words, N, [theta], carried=9)
    assert np.array_equal(part, lpc[:, 9:]) and np.array_equal(pc, cnt[9:])


def _rings(rng, cap, R, H, split, h_scale=2.0 ** 14):
    """random rings in either state-row format, as torch tensors (the double reads them through their pointers)"""
    import torch
    x = rng.uniform(-1, 1, size=(cap, R, H)).astype(np.float32)
    if split:
        s = x * np.float32(h_scale)
        hi = s.astype(np.float16)
        lo = (s - hi.astype(np.float32)).astype(np.float16)
        raw = np.stack([hi.reshape(cap, R, H // 8, 8), lo.reshape(cap, R, H // 8, 8)], axis=3).reshape(cap, R, 2 * H).view(np.float32)
        x = ((hi.astype(np.float64) + lo.astype(np.float64)) / h_scale)
    else:
        raw = x
    return torch.from_numpy(np.ascontiguousarray(raw)), x.astype(np.float64)


@pytest.mark.parametrize("split", [0, 1])
def test_theta_zero_counts_at_the_windows_edges(fake, split):
    """theta = 0: lpc = log(#matches / n_q).  The one matching entry is moved across the window's old edge (q - N counts, q - N - 1
    does not) and across ``first``, with the ring wrapped"""
    import torch
    rng = np.random.RandomState(3)
    cap, R, H, N, nq, pos0 = 16, 2, 32, 5, 4, 29                     # positions 24 .. 32 in slots 8 .. 15, 0: the window wraps
    hist, _x = _rings(rng, cap, R, H, split)
    lib = _lib.lib()
    th = (ctypes.c_float * 1)(0.0)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)

    def run(match_pos, first):
        words = np.full((cap, R), 7, dtype=np.int32)
        for q in range(nq):
            words[(pos0 + q) % cap] = 100 + q                          # every query its own word
        words[match_pos % cap, :] = 100 + 2                            # ... and one entry matching query 2 (position 31)
        lpc = torch.full((1, nq, R), 5.0)
        flags = torch.zeros(1, dtype=torch.int32)
        wd, fs, ln = i32(words), i32(first), i32([nq, nq])              # (kept alive across the call: the double reads their pointers)
        rc = lib.jlm_cache_rows(hist.data_ptr(), wd.data_ptr(), cap, R, H, split, 2.0 ** 14, pos0, nq, fs.data_ptr(), ln.data_ptr(), N, th, 1,
                                lpc.data_ptr(), flags.data_ptr(), 0)
        assert rc == 0 and int(flags[0]) == 0
        return lpc.numpy()[0]

    q2 = pos0 + 2
    got = run(q2 - N, [0, 0])                                          # the oldest entry of the window counts
    assert got[2, 0] == pytest.approx(np.log(1 / N), abs=1e-6) and np.all(np.isinf(got[[0, 1, 3]]))
    assert np.all(np.isinf(run(q2 - N - 1, [0, 0])))                   # one older does not
    got = run(q2 - 3, [q2 - 3, q2 - 2])                                # first: row 0 starts AT the entry, row 1 one behind it
    assert got[2, 0] == pytest.approx(np.log(1 / 3), abs=1e-6) and got[2, 1] == -np.inf


# ---------------------------------------------------------------------------------------------- the host path over the double
def _stream(V, B=3, n=45, seed=11):
    """B streams of n steps whose words repeat (a vocabulary of a dozen words): matches everywhere"""
    rng = np.random.RandomState(seed)
    pool = rng.randint(2, V, size=12)
    s = pool[rng.randint(0, 12, size=(B, n + 1))].astype(np.int32)
    return s[:, :-1], s[:, 1:]


def _run_cut(m, x, y, spec, cuts):
    h = c = state = None
    parts = []
    at = 0
    for k in cuts:
        res = m.score_streams_cached(x[:, at:at + k], y[:, at:at + k], spec, h, c, state)
        h, c, state = res.h, res.c, res.state
        parts.append(res)
        at += k
    assert at == x.shape[1]
    return (np.concatenate([p.nll_lm for p in parts], axis=1), np.concatenate([p.logp_cache for p in parts], axis=2),
            np.concatenate([p.n_entries for p in parts], axis=1), state)


@pytest.mark.parametrize("name", ["tied", "untied"])
@pytest.mark.parametrize("N", [16, 64])
def test_cutting_invariance_and_reference(name, N, fake):
    m = _model(name)
    x, y = _stream(cc.MODELS[name][0])
    spec = C.CacheSpec(N, theta=[0.0, 0.5, 2.0], lam=0.2)
    nll, lpc, cnt, state = _run_cut(m, x, y, spec, [45])
    assert lpc.shape == (3, 3, 45) and cnt.shape == (3, 45) and nll.shape == (3, 45)
    assert np.array_equal(cnt, np.broadcast_to(np.minimum(np.arange(45), N), (3, 45)))
    for cuts in ([20, 20, 5], [1] * 45):
        nll2, lpc2, cnt2, state2 = _run_cut(m, x, y, spec, cuts)
        assert np.array_equal(cnt2, cnt)
        np.testing.assert_allclose(nll2, nll, rtol=0, atol=1e-9)
        both = np.isfinite(lpc)
        assert np.array_equal(np.isfinite(lpc2), both)
        np.testing.assert_allclose(lpc2[both], lpc[both], rtol=0, atol=2e-6)          # float32 outputs of float64 sums
        assert state2.pos == state.pos == 45 and state2.count == state.count == min(45, N)
    # the reference over the states the call itself kept (N >= the stream: every state)
    full = m.score_streams_cached(x, y, C.CacheSpec(64, theta=[0.0, 0.5, 2.0]))
    h, words, pos = full.state.numpy()
    assert h.shape == (3, 45, cc.MODELS[name][1]) and np.array_equal(words, y) and np.array_equal(pos, np.arange(45))
    for b in range(3):
        want, wc = C.cache_log_probs(h[b], words[b], N, spec.thetas)
        assert np.array_equal(wc, cnt[b])
        assert np.array_equal(np.isfinite(want), np.isfinite(lpc[:, b]))
        ok = np.isfinite(want)
        np.testing.assert_allclose(lpc[:, b][ok], want[ok], rtol=0, atol=2e-6)
    assert np.isfinite(lpc).any() and np.any(lpc[:, :, 1:] == -np.inf)          # matches and misses both occur
    # theta = 0 through the whole path: log(#matches / n_q)
    for b in range(3):
        for q in range(1, 45):
            lo = max(q - N, 0)
            k = int(np.sum(y[b, lo:q] == y[b, q]))
            want = np.log(k / (q - lo)) if k else -np.inf
            assert lpc[0, b, q] == pytest.approx(want, abs=1e-6)


def test_mixture(fake):
    m = _model("tied")
    x, y = _stream(cc.MODELS["tied"][0])
    res = m.score_streams_cached(x, y, C.CacheSpec(16, theta=[0.5, 1.0], lam=0.3))
    assert res.nll(0).tobytes() == res.nll_lm.tobytes() and res.nll(0, 1).tobytes() == res.nll_lm.tobytes()
    for lam in (0.05, 0.3, 0.95):
        for t in (0, 1):
            got = res.nll(lam, t)
            lpc = res.logp_cache[t]
            empty = res.n_entries == 0
            assert empty[:, 0].all() and np.array_equal(got[empty], res.nll_lm[empty])           # no entry: the model alone
            miss = ~empty & np.isinf(lpc)
            assert miss.any()
            np.testing.assert_allclose(got[miss], res.nll_lm[miss] - np.log1p(-lam), rtol=0, atol=1e-12)
            hit = ~empty & ~miss
            want = -np.log((1 - lam) * np.exp(-res.nll_lm[hit]) + lam * np.exp(lpc[hit]))
            np.testing.assert_allclose(got[hit], want, rtol=0, atol=1e-10)
    for bad in (-0.1, 1.0, 1.5, True, None, "0.1", float("nan")):
        with pytest.raises(ValueError):
            res.nll(bad)
    with pytest.raises(ValueError):
        res.nll(0.1, 2)


def test_score_cached_sequences(fake):
    """ragged sequences, empty ones included: every sequence from an empty cache, whatever the row plan"""
    m = _model("tied")
    V = cc.MODELS["tied"][0]
    rng = np.random.RandomState(2)
    pool = rng.randint(2, V, size=6)
    seqs = [list(pool[rng.randint(0, 6, size=L)]) for L in (9, 0, 30, 1, 17, 0, 30)]
    spec = C.CacheSpec(8, theta=0.7, lam=0.25)
    got = m.score_cached(seqs, cc.EOS, spec)
    assert [len(g) for g in got] == [len(s) for s in seqs] and all(g.dtype == np.float64 for g in got)
    for s, g in zip(seqs, got):
        if not len(s):
            continue
        one = m.score_streams_cached(np.array([[cc.EOS] + s[:-1]]), np.array([s]), spec)
        np.testing.assert_allclose(g, one.nll(spec.lam)[0], rtol=0, atol=1e-6)
    for max_rows in (1, 2):
        again = m.score_cached(seqs, cc.EOS, spec, max_rows=max_rows)
        assert all(np.allclose(a, b, rtol=0, atol=1e-6) for a, b in zip(got, again))
    assert m.score_cached([], cc.EOS, spec) == []


def test_row_budget_shrinks_with_the_cache(fake):
    from jlm_amd.rowsets import clamp_rows
    from jlm_amd.score import MAX_ROWS, SCORE_BUDGET_BYTES
    sc = _model("tied-h512")._scorer()
    plain = sc.row_bytes(20)
    assert sc.row_bytes(20, True, 0) == plain
    for N in (500, 2000, 100000):
        assert sc.row_bytes(20, True, N) >= plain + (N + 20) * 512 * 4
    assert clamp_rows(MAX_ROWS, SCORE_BUDGET_BYTES, sc.row_bytes(20, True, 100000), 512) * (100020 * 512 * 4) <= SCORE_BUDGET_BYTES
    assert clamp_rows(MAX_ROWS, SCORE_BUDGET_BYTES, sc.row_bytes(20, True, 100000), 512) < MAX_ROWS


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(size=0), dict(size=-3), dict(size=2.0), dict(size=True), dict(size=None), dict(theta=-0.1),
                                dict(theta=float("nan")), dict(theta=float("inf")), dict(theta=[]), dict(theta=[0.1] * 17),
                                dict(theta=[0.1, -1]), dict(theta="x"), dict(theta=True), dict(lam=1.0), dict(lam=-0.01),
                                dict(lam=float("nan")), dict(lam=None), dict(lam=True)])
def test_spec_refuses(kw):
    args = dict(size=10, theta=0.3, lam=0.1)
    args.update(kw)
    with pytest.raises(ValueError):
        C.CacheSpec(**args)


def test_spec_accepts():
    s = C.CacheSpec(1, theta=[0, 0.5], lam=0)
    assert (s.size, s.thetas, s.theta, s.lam) == (1, (0.0, 0.5), 0.0, 0.0)
    assert C.CacheSpec(5, np.float32(0.25), np.float64(0.5)).thetas == (0.25,)
    assert len(C.CacheSpec(5, np.linspace(0, 1, 16)).thetas) == 16


def test_refusals_launch_nothing(fake):
    import torch
    m = _model("tied")
    other = _model("untied")
    V = cc.MODELS["tied"][0]
    x, y = _stream(V, n=6)
    spec = C.CacheSpec(4)
    ok = m.score_streams_cached(x, y, spec)
    foreign = other.score_streams_cached(x, y, spec).state
    del fake.launches[:]
    bad_y = y.copy()
    bad_y[1, 2] = V
    for a, kw in (((x, y[:, :5], spec), {}), ((x[0], y[0], spec), {}), ((x, bad_y, spec), {}), ((-x, y, spec), {}),
                  ((x, y, None), {}), ((x, y, (4, 0.3, 0.1)), {}), ((x, y, spec), dict(h=ok.h)), ((x, y, spec), dict(state=foreign)),
                  ((x[:2], y[:2], spec), dict(state=ok.state)), ((x, y, spec), dict(state=object())),
                  ((x, y, spec), dict(h=torch.zeros(2, 64), c=torch.zeros(2, 64)))):
        with pytest.raises(ValueError):
            m.score_streams_cached(*a, **kw)
    for kw in (dict(sequences=[[1, V]]), dict(start=-1), dict(cache=None), dict(max_rows=0)):
        args = dict(sequences=[[2, 3]], start=cc.EOS, cache=spec)
        args.update(kw)
        with pytest.raises(ValueError):
            m.score_cached(**args)
    assert fake.launches == []
    empty = m.score_streams_cached(x[:, :0], y[:, :0], spec, state=ok.state)
    assert empty.nll_lm.shape == (3, 0) and empty.logp_cache.shape == (1, 3, 0) and empty.state is ok.state
    assert [len(g) for g in m.score_cached([[], []], cc.EOS, spec)] == [0, 0]
    assert fake.launches == []


def test_launcher_refusals(fake):
    """the header's refusals of jlm_cache_rows, each -1 with nothing launched; empty shapes return 0 with nothing launched"""
    import torch
    rng = np.random.RandomState(0)
    cap, R, H, N, nq = 12, 2, 32, 4, 8
    hist, _x = _rings(rng, cap, R, H, 0)
    words = torch.zeros((cap, R), dtype=torch.int32)
    first = torch.zeros(R, dtype=torch.int32)
    length = torch.full((R,), nq, dtype=torch.int32)
    lpc = torch.zeros((1, nq, R))
    th = (ctypes.c_float * 17)(*([0.5] * 17))
    neg = (ctypes.c_float * 1)(-1.0)
    lib = _lib.lib()
    base = dict(hist=hist.data_ptr(), words=words.data_ptr(), cap=cap, n_rows=R, H=H, split=0, h_scale=1.0, pos0=0, n_query=nq,
                first=first.data_ptr(), length=length.data_ptr(), N=N, thetas=th, n_theta=1, lpc=lpc.data_ptr(), flags=None, stream=0)
    call = lambda **kw: lib.jlm_cache_rows(**dict(base, **kw))
    del fake.launches[:]
    for kw in (dict(cap=N + nq - 1), dict(H=0), dict(H=48), dict(H=-32), dict(hist=hist.data_ptr() + 4), dict(words=words.data_ptr() + 2),
               dict(hist=None), dict(lpc=None), dict(n_theta=0), dict(n_theta=17), dict(thetas=neg), dict(N=0), dict(pos0=-1),
               dict(pos0=0x7fffffff - 10), dict(split=1, h_scale=0.0), dict(n_rows=-1)):
        assert call(**kw) == -1, kw
    assert call(n_rows=0) == 0 and call(n_query=0, cap=N) == 0
    assert fake.launches == []
    assert call() == 0 and fake.launches == ["cache_rows"]


# ---------------------------------------------------------------------------------------------- the tuner
def _scores(nll, lpc, cnt, thetas):
    return C.CachedScores(np.asarray(nll, dtype=np.float64), np.asarray(lpc, dtype=np.float64), np.asarray(cnt), thetas, None, None, None)


def test_tune_picks_the_grid_minimum():
    rng = np.random.RandomState(4)
    thetas = (0.0, 0.5, 1.0)
    parts = []
    for _ in range(3):
        nll = rng.uniform(1, 6, size=(2, 10))
        lpc = np.log(rng.uniform(1e-3, 1, size=(3, 2, 10)))
        lpc[1] += 0.8                                                   # theta 0.5 is the best cache
        lpc[:, rng.rand(2, 10) < 0.2] = -np.inf
        parts.append(_scores(nll, np.minimum(lpc, 0), rng.randint(0, 3, size=(2, 10)), thetas))
    lams = [0.0, 0.1, 0.2, 0.4, 0.8]
    grid = C.perplexity_grid(parts, lams)
    assert grid.shape == (3, 5)
    want = np.zeros((3, 5))
    for t in range(3):
        for j, lam in enumerate(lams):
            tot = 0.0
            for p in parts:
                pm = np.exp(-p.nll_lm)
                mix = np.where(p.n_entries > 0, (1 - lam) * pm + lam * np.exp(p.logp_cache[t]), pm)
                tot += -np.log(mix).sum()
            want[t, j] = np.exp(tot / 60)
    np.testing.assert_allclose(grid, want, rtol=1e-12)
    theta, lam = C.tune(parts, lams)
    t, j = np.unravel_index(np.argmin(want), want.shape)
    assert (theta, lam) == (thetas[t], lams[j]) and theta == 0.5 and lam > 0
    assert np.all(grid[:, 0] == grid[0, 0])                             # lam = 0: the model's perplexity whatever theta
    assert C.tune(parts[0], lams) == C.tune([parts[0]], lams)
    # a useless cache: lam = 0 wins
    useless = _scores(np.ones((1, 4)), np.full((2, 1, 4), -np.inf), np.ones((1, 4), dtype=int), (0.0, 1.0))
    assert C.tune(useless, [0.0, 0.5]) == (0.0, 0.0)
    for bad in (([], lams), (parts, []), (parts, [1.0]), ([parts[0], useless], lams)):
        with pytest.raises(ValueError):
            C.tune(*bad)


# ---------------------------------------------------------------------------------------------- the command line
def _write_corpus(root, name, lines):
    with open(os.path.join(root, "data", name), "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return os.path.join(root, "data", name)


def _passage_corpus(root):
    """one 30-word passage repeated: 24 lines of the same 29 words (+ <eos> each)"""
    from jlm_amd.data import Vocab
    cc.set_root("tied")
    vocab = Vocab(cc.MODELS["tied"][0])
    words = [w for w in vocab.t2i if w not in ("<unk>", "<eos>")]
    rng = np.random.RandomState(8)
    passage = " ".join(words[i] for i in rng.choice(len(words), size=29, replace=False))
    return [passage] * 24


def test_command_line(fake, capsys):
    from jlm_amd import perplexity
    lines_of = lambda: [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("LSTM model:")]     # (the loader's own line)
    root = cc.model_root("tied")
    os.makedirs(os.path.join(root, "data"), exist_ok=True)
    lines = _passage_corpus(root)
    path = _write_corpus(root, "cache_test.txt", lines)
    dev = _write_corpus(root, "cache_dev.txt", lines[:12])
    common = ["--root", root, "-e", "1", "--mode", "stream", "-b", "2", "--num_steps", "10", "--file", path]
    # without --cache: the plain path (LSTM_Model.score_streams) is what runs, and prints what it printed
    calls = []
    monkey_pp = perplexity.stream_perplexity
    perplexity.stream_perplexity = lambda *a: calls.append(a[2:]) or (7.5, 1.0, 10)
    try:
        assert perplexity.main(common) == 7.5
    finally:
        perplexity.stream_perplexity = monkey_pp
    out = lines_of()
    assert calls == [(2, 10)] and len(out) == 2 and out[0].startswith("tokens: 10  <unk>: 0  tokens/s: ") and out[1] == "Test perplexity: 7.5"
    # with --cache: the plain perplexity, then a lower cached one
    pp = perplexity.main(common + ["--cache", "40", "--theta", "0.5", "--lam", "0.2"])
    out = lines_of()
    assert len(out) == 3 and out[1] == "Test perplexity: {}".format(pp)
    assert out[2].startswith("Test perplexity with cache (N 40 theta 0.5 lam 0.2): ")
    cached = float(out[2].rsplit(" ", 1)[1])
    assert cached < pp
    # the tuner: the grid's best pair, the test perplexity at that pair -- no worse than any pair tried by hand on the same text
    pp2 = perplexity.main(common + ["--cache", "40", "--tune-cache", dev, "--thetas", "0,0.5,2", "--lams", "0,0.2,0.6"])
    out = lines_of()
    assert pp2 == pp and len(out) == 4 and out[2].startswith("Cache tuned on {}: theta ".format(dev))
    assert out[3].startswith("Test perplexity with cache (N 40 theta ") and float(out[3].rsplit(" ", 1)[1]) < pp
    for bad in (["--cache", "0", "--tune-cache", dev], ["--cache", "8", "--mode", "sentence"], ["--cache", "8", "--lam", "1"],
                ["--cache", "8", "--theta", "-1"], ["--cache", "8", "--tune-cache", dev, "--lams", "0,2"], ["--tune-cache", dev]):
        with pytest.raises(SystemExit):
            perplexity.main(common + bad)
    capsys.readouterr()


# ---------------------------------------------------------------------------------------------- the exports
def test_lib_exposes_the_cache_entries():
    assert "jlm_cache_rows" in _lib.EXPORTS and "jlm_score_cache_frames" in _lib.EXPORTS
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "jlm_cache_rows") and hasattr(lib, "jlm_score_cache_frames")
    names = [f[0] for f in _lib.CachePlan._fields_]
    assert names == ["hist", "words", "cap", "pos0", "first", "len", "N", "thetas", "n_theta", "lpc", "flags"]
    assert [f[0] for f in _lib.ScorePlan._fields_][:2] == ["n_rows", "n_steps"] and len(_lib.ScorePlan._fields_) == 18     # unchanged
