"""CPU: ranking and prediction under a memory (jlm_amd/memory.py MemoryMix / Memory.search / rank_streams_memory / rank_memory /
predict_next_memory): the float64 definition, the refusals, and the host path of the three entry points over the
numpy double of tests/fake_memory_topk.py, which restates the header's contract.  The kernels run in tests/test_gpu_memory_topk.py and
tests/test_gpu_rank_memory.py."""
import ctypes
import os

import numpy as np
import pytest

from jlm_amd import _lib, cache as C, memory as M
from tests import context_cases as cc
from tests import fake_memory_topk
from tests.test_memory_cpu import _model, _streams, _write, build_order, oracle_states

MAX_PREFIX = 3


@pytest.fixture()
def fake(monkeypatch):
    return fake_memory_topk.install(monkeypatch)


# ---------------------------------------------------------------------------------------------- the definition
def test_neighbours_order_and_exact_ties():
    """larger s first, smaller index first among equal s -- also at theta = 0, where every entry ties, and with -0 products"""
    q = np.array([1.0, 0.0, 0.0, 0.0])
    keys = np.array([[0.5, 0, 0, 0], [2.0, 0, 0, 0], [0.5, 1, 0, 0], [-1.0, 0, 0, 0], [2.0, 0, 3, 0], [0.0, 7, 0, 0], [0.5, 0, 0, 9]])
    idx, s = M.memory_neighbours(q, keys, 0.5, 1024)
    assert idx.tolist() == [1, 4, 0, 2, 6, 5, 3] and idx.dtype == np.int64 and s.tolist() == [1.0, 1.0, 0.25, 0.25, 0.25, 0.0, -0.5]
    for k in range(1, 8):
        i2, s2 = M.memory_neighbours(q, keys, 0.5, k)
        assert i2.tolist() == idx[:k].tolist() and s2.tolist() == s[:k].tolist()
    idx, s = M.memory_neighbours(q, keys, 0.0, 5)
    assert idx.tolist() == [0, 1, 2, 3, 4] and np.all(s == 0) and not np.signbit(s).any()          # 0 * -1 is one zero, one tie
    rng = np.random.RandomState(3)
    keys = rng.randn(200, 8)[rng.randint(0, 20, size=200)]                                       # exact duplicates
    q = rng.randn(8)
    idx, s = M.memory_neighbours(q, keys, 1.3, 50)
    full = 1.3 * (keys @ q)
    assert np.all(np.diff(s) <= 0) and np.array_equal(s, full[idx])
    assert all(a < b for a, b, sa, sb in zip(idx[:-1], idx[1:], s[:-1], s[1:]) if sa == sb)
    rest = np.setdiff1d(np.arange(200), idx)
    assert full[rest].max() <= s[-1] and np.all(rest[full[rest] == s[-1]] > idx[s == s[-1]].max())
    for bad in (0, 1025, 2.5):
        with pytest.raises(ValueError):
            M.memory_neighbours(q, keys, 1.0, bad)
    with pytest.raises(ValueError):
        M.memory_neighbours(q[:4], keys, 1.0, 3)


@pytest.mark.parametrize("theta", [0.0, 0.4, 3.0])
def test_distribution_with_every_entry_is_the_scored_memory(theta):
    """K >= N: memory_distribution at the target equals exp(memory_log_probs); any K: c sums to 1 over the retrieved words"""
    rng = np.random.RandomState(5)
    N, H, V = 57, 16, 9
    keys, words = rng.randn(N, H) * 0.5, rng.randint(0, 7, size=N)
    hq, wq = rng.randn(6, H) * 0.5, rng.randint(0, 9, size=6)
    lpm = M.memory_log_probs(hq, wq, keys, words, [theta])[0]
    for q in range(6):
        c = M.memory_distribution(hq[q], keys, words, theta, 64, V)
        assert c.shape == (V,) and abs(c.sum() - 1) < 1e-12
        with np.errstate(divide="ignore"):
            assert np.log(c[wq[q]]) == pytest.approx(lpm[q], abs=1e-12) if np.isfinite(lpm[q]) else c[wq[q]] == 0
        c5 = M.memory_distribution(hq[q], keys, words, theta, 5, V)
        idx, s = M.memory_neighbours(hq[q], keys, theta, 5)
        assert abs(c5.sum() - 1) < 1e-12 and set(np.flatnonzero(c5).tolist()) == set(words[idx].tolist())
        e = np.exp(s - s.max())
        assert c5[words[idx[0]]] == pytest.approx(e[words[idx] == words[idx[0]]].sum() / e.sum(), abs=1e-15)
    with pytest.raises(ValueError):
        M.memory_distribution(hq[0], keys, words, theta, 5, 6)                                   # a word outside [0, V)


# ---------------------------------------------------------------------------------------------- the host path over the double
def _cut(m, x, y, mix, cuts, top=5):
    h = c = None
    parts, at = [], 0
    for k in cuts:
        res = m.rank_streams_memory(x[:, at:at + k], y[:, at:at + k], mix, h, c, max_prefix=MAX_PREFIX, top=top, neighbours=True)
        h, c = res.h, res.c
        parts.append(res)
        at += k
    return (np.concatenate([p.ranks for p in parts], axis=1), np.concatenate([p.top_ids for p in parts], axis=1),
            np.concatenate([p.top_logp for p in parts], axis=1), np.concatenate([p.neighbours for p in parts], axis=1), h, c)


@pytest.mark.parametrize("name", list(cc.MODELS))
def test_streams_sequences_and_prediction(name, fake):
    m = _model(name)
    dm = m.dev
    (xm, ym), (x, y) = _streams(dm.V, n=24)
    B, n = x.shape
    memory = M.Memory.build(m, xm, ym, 10)
    plain, hp, cp = m.rank_streams(x, y, max_prefix=MAX_PREFIX)
    ora_k = build_order(oracle_states(name, xm, ym)[0], 10)
    k_words = build_order(ym, 10).astype(np.int64)
    ora_h = oracle_states(name, x, y)[0]
    for K in (5, 1024):
        mix = M.MemoryMix(memory, theta=0.5, lam=0.2, k=K)
        n_q = min(K, memory.N)
        del fake.launches[:]
        ranks, ids, logp, nb, h, c = _cut(m, x, y, mix, [24])
        assert fake.launches.count("rank_memory_frames") == 1 and fake.launches.count("memory_topk") == n
        assert ranks.shape == plain.shape and ids.shape == (B, n, 5) and nb.shape == (B, n, n_q) and nb.dtype == np.int64
        assert np.array_equal(h.numpy(), hp.numpy()) and np.array_equal(c.numpy(), cp.numpy())
        for cuts in ([10, 10, 4], [3, 21]):                                # a stream cut any way: the same bits
            r2, i2, l2, n2, _h, _c = _cut(m, x, y, mix, cuts)
            assert np.array_equal(r2, ranks) and np.array_equal(i2, ids) and l2.tobytes() == logp.tobytes() and np.array_equal(n2, nb)
        # the neighbours are the definition's over the double's own states, up to the ties float32 scores add; as sets for K >= N
        dev_k = memory.numpy()[0].astype(np.float64)
        for b in range(B):
            for q in range(n):
                got = nb[b, q]
                assert len(set(got.tolist())) == n_q
                if K >= memory.N:
                    assert set(got.tolist()) == set(range(memory.N))
                else:
                    s64 = 0.5 * (ora_k @ ora_h[b, q])
                    rest = np.setdiff1d(np.arange(memory.N), got)
                    assert s64[rest].max() <= s64[got].min() + 1e-4
                assert (ranks[b, q, 0] < 5) == (int(y[b, q]) in ids[b, q])
        assert np.array_equal(k_words, memory.numpy()[1]) and dev_k.shape == ora_k.shape
        assert np.any(ranks[:, :, 0] != plain[:, :, 0])
        present = np.isin(y, ym)
        assert ranks[:, :, 0][present].mean() < plain[:, :, 0][present].mean()
        # the one-step form: the loop's next-step list from the carried state
        first = m.rank_streams_memory(x[:, :9], y[:, :9], mix, max_prefix=MAX_PREFIX)
        step = m.rank_streams_memory(x[:, 9:10], y[:, 9:10], mix, first.h, first.c, max_prefix=MAX_PREFIX, top=5)
        if dm.mode == "untied" and dm.split_lstm:
            with pytest.raises(ValueError, match="untied split-row"):
                m.predict_next_memory(step.h, mix, n=5)
        else:
            got = m.predict_next_memory(step.h, mix, n=5)
            for b in range(B):
                assert np.array_equal(got[b][0], step.top_ids[b, 0]) and got[b][1].tobytes() == step.top_logp[b, 0].tobytes()
        # Memory.search over the carried state: the step's neighbours
        step_nb = m.rank_streams_memory(x[:, 9:10], y[:, 9:10], mix, first.h, first.c, readings=False, neighbours=True)
        idx, sc, words = memory.search(step_nb.h, K, 0.5)
        assert np.array_equal(idx, step_nb.neighbours[:, 0]) and np.array_equal(words, k_words[idx]) and sc.dtype == np.float32
        assert np.all(np.diff(sc, axis=1) <= 0)
    # lam = 0: rank_streams' array, and nothing patched
    del fake.launches[:]
    zero = m.rank_streams_memory(x, y, M.MemoryMix(memory, theta=0.5, lam=0.0, k=5), max_prefix=MAX_PREFIX)
    assert np.array_equal(zero.ranks, plain) and zero.top_ids is None and zero.neighbours is None and "cache_mix_rows" not in fake.launches
    # ragged sequences in rank()'s row plan: every sequence ranks as its own stream, whatever the chunking
    mix = M.MemoryMix(memory, theta=0.7, lam=0.25, k=5)
    seqs = [[int(w) for w in y[i % 3, :L]] for i, L in enumerate((9, 0, 20, 1, 17, 0))]
    got = m.rank_memory(seqs, 1, mix, max_prefix=MAX_PREFIX)
    cut = m.rank_memory(seqs, 1, mix, max_prefix=MAX_PREFIX, max_rows=2)
    for s, g, g2 in zip(seqs, got, cut):
        assert g.shape == (len(s), MAX_PREFIX + 3) and np.array_equal(g, g2)
        if len(s):
            one = m.rank_streams_memory(np.array([[1] + s[:-1]]), np.array([s]), mix, max_prefix=MAX_PREFIX)
            assert np.array_equal(one.ranks[0], g)
    empty = m.rank_streams_memory(x[:, :0], y[:, :0], mix, max_prefix=MAX_PREFIX, top=3, neighbours=True)
    assert empty.ranks.shape == (B, 0, MAX_PREFIX + 3) and empty.neighbours.shape == (B, 0, 5)


# ---------------------------------------------------------------------------------------------- refusals
def test_mix_and_search_refusals(fake):
    m = _model("tied")
    (xm, ym), (x, y) = _streams(m.dev.V, n=6)
    memory = M.Memory.build(m, xm, ym, 6)
    mix = M.MemoryMix(memory)
    assert (mix.theta, mix.lam, mix.k, mix.n_q) == (0.3, 0.1, 64, 18)
    for bad in (dict(k=0), dict(k=1025), dict(k=True), dict(k=2.5), dict(theta=[0.1, 0.2]), dict(theta=-1.0), dict(theta=float("nan")),
                dict(lam=1.0), dict(lam=-0.1)):
        with pytest.raises(ValueError):
            M.MemoryMix(memory, **bad)
    for bad in (None, M.MemorySpec(), "memory"):
        with pytest.raises(ValueError):
            M.MemoryMix(bad)
    other = _model("vtable")
    del fake.launches[:]
    with pytest.raises(ValueError, match="of this model"):
        other.rank_streams_memory(x, y, mix, readings=False)
    with pytest.raises(ValueError, match="of this model"):
        other.rank_memory([[3, 4]], 1, mix, readings=False)
    res = m.rank_streams_memory(x, y, mix, readings=False)
    del fake.launches[:]
    with pytest.raises(ValueError, match="of this model"):
        other.predict_next_memory(res.h, mix)
    with pytest.raises(ValueError, match="MemoryMix"):
        m.rank_streams_memory(x, y, M.MemorySpec(), readings=False)
    with pytest.raises(ValueError, match="top"):
        m.rank_streams_memory(x, y, mix, readings=False, top=65)
    with pytest.raises(ValueError):
        m.predict_next_memory(res.h, mix, n=0)
    for bad in (dict(k=0), dict(k=1025), dict(k=4, theta=-1.0)):
        with pytest.raises(ValueError):
            memory.search(res.h, **bad)
    with pytest.raises(ValueError):
        memory.search(res.h[:, :8], 4)
    with pytest.raises(ValueError):
        memory.search(None, 4)
    assert fake.launches == []                                             # every refusal before anything runs
    idx, sc, words = memory.search(res.h[:0], 4)
    assert idx.shape == sc.shape == words.shape == (0, 4) and fake.launches == []


def test_launcher_refusals_and_workspace(fake):
    """the double's launcher restates the header's refusals; the package sizes the workspace as the launcher reads it"""
    lib = fake
    assert lib.jlm_memory_topk_workspace_bytes(1000, 3, 64) == 3 * (128 + 512) and lib.jlm_memory_topk_workspace_bytes(0, 3, 64) == 0
    assert lib.jlm_memory_topk_workspace_bytes(1000, 3, 1025) == 0
    for N, R, K in ((1, 1, 1), (1000, 3, 64), (10 ** 6, 1024, 1024), (1 << 24, 64, 64)):
        floats = M.RetrievalBuffers.workspace_floats(N, R, K)
        chunk = M.RetrievalBuffers.chunk_keys(N, R)
        assert chunk % 32 == 0 and 32 <= chunk <= -(-N // 32) * 32 and 4 * R * chunk <= max(M.TOPK_SCORE_BYTES, 128 * R)
        assert lib.jlm_memory_topk_chunk_keys(N, R, K, 4 * floats) == chunk
    keys = np.zeros((40, 32), dtype=np.float32)
    kw = np.zeros(40, dtype=np.int32)
    q = np.zeros((2, 32), dtype=np.float32)
    s = np.full((2, 8), 9.0, dtype=np.float32)
    rw = np.full((7, 2), -7, dtype=np.int32)
    ri = np.full((7, 2), -7, dtype=np.int32)
    ws = np.zeros(2 * (32 + 14), dtype=np.float32)
    a = dict(keys=keys.ctypes.data, key_words=kw.ctypes.data, N=40, H=32, split=0, h_scale=1.0, q_rows=q.ctypes.data, n_rows_max=2, n_dev=None,
             theta=0.5, K=7, s=s.ctypes.data, ld_s=8, ret_words=rw.ctypes.data, ret_idx=ri.ctypes.data, n_rows=2, workspace=ws.ctypes.data,
             workspace_bytes=ws.nbytes, flags=None, stream=0)
    for kw_ in (dict(N=0), dict(N=(1 << 24) + 1), dict(H=48), dict(K=0), dict(K=1025), dict(ld_s=6), dict(theta=-1.0), dict(n_rows_max=3),
                dict(keys=None), dict(s=None), dict(ret_words=None), dict(workspace=None), dict(workspace_bytes=ws.nbytes - 4)):
        assert lib.jlm_memory_topk(*dict(a, **kw_).values()) == -1, kw_
    assert np.all(s == 9.0) and np.all(rw == -7) and lib.launches == []
    assert lib.jlm_memory_topk(*dict(a, n_rows_max=0).values()) == 0 and lib.launches == []
    assert lib.jlm_memory_topk(*a.values()) == 0 and lib.launches == ["memory_topk"]
    assert np.array_equal(ri, np.repeat(np.arange(7)[:, None], 2, axis=1)) and np.all(s[:, :7] == 0) and np.all(s[:, 7] == 9.0)


# ---------------------------------------------------------------------------------------------- the command line
def test_command_line_with_and_without_mem_k(fake, capsys, tmp_path):
    from jlm_amd import perplexity
    from jlm_amd.data import Vocab
    lines_of = lambda: [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("LSTM model:")]
    root = cc.model_root("tied")
    cc.set_root("tied")
    os.makedirs(os.path.join(root, "data"), exist_ok=True)
    vocab = Vocab(cc.MODELS["tied"][0])
    words = [w for w in vocab.t2i if w not in ("<unk>", "<eos>")]
    rng = np.random.RandomState(8)
    passage = " ".join(words[i] for i in rng.choice(len(words), size=29, replace=False))
    text = _write(root, "memory_rank_text.txt", [passage] * 6)
    test = _write(root, "memory_rank_test.txt", [passage] * 4)
    mem_path = str(tmp_path / "mem.npz")
    model_args = ["--root", root, "-e", "1"]
    M.main(model_args + ["--text", text, "-b", "2", "--num_steps", "10", "--out", mem_path])
    lines_of()
    common = model_args + ["--mode", "stream", "-b", "2", "--num_steps", "10", "--file", test, "--ranks", "--memory", mem_path,
                           "--mem-theta", "0.5", "--mem-lam", "0.2"]
    del fake.launches[:]
    perplexity.main(common)
    before = lines_of()
    assert "rank_memory_frames" not in fake.launches and not any(ln.startswith("with memory") for ln in before)
    perplexity.main(common + ["--mem-k", "8"])
    out = lines_of()
    strip = lambda lines: [ln.split("  tokens/s")[0] for ln in lines]
    assert len(out) == len(before) + 1 and strip(out[:-1]) == strip(before) and "rank_memory_frames" in fake.launches
    assert out[-1].startswith("with memory (N 160 K 8 theta 0.5 lam 0.2): top-1: ")     # 6 lines of 30 tokens in 2 streams of 8 x 10 steps
    mrr = lambda line: float(line.split("MRR: ")[1].split()[0])
    plain_line = [ln for ln in out if ln.startswith("top-1:")]
    assert len(plain_line) == 1 and mrr(out[-1]) > mrr(plain_line[0])                            # a repeated passage: the memory lifts it
    for bad in (["--mem-k", "0"], ["--mem-k", "1025"]):
        with pytest.raises(SystemExit):
            perplexity.main(common + bad)
    with pytest.raises(SystemExit):
        perplexity.main(model_args + ["--mode", "stream", "-b", "2", "--num_steps", "10", "--file", test, "--ranks", "--mem-k", "8"])
    with pytest.raises(SystemExit):
        perplexity.main([a for a in common if a != "--ranks"] + ["--mem-k", "8"])
    capsys.readouterr()


# ---------------------------------------------------------------------------------------------- the exports
def test_lib_exposes_the_retrieval_entries():
    names = ("jlm_memory_topk", "jlm_memory_topk_workspace_bytes", "jlm_memory_topk_chunk_keys", "jlm_rank_memory_frames",
             "jlm_predict_memory_rows")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(n in _lib.EXPORTS and hasattr(lib, n) for n in names)
    assert [f[0] for f in _lib.MemoryMixPlan._fields_] == ["keys", "key_words", "N", "theta", "lam", "K", "s", "ld_s", "ret_words", "ret_idx",
                                                           "keep_idx", "first", "workspace", "workspace_bytes", "top_k", "top_ids", "top_nll",
                                                           "flags"]
    assert len(_lib.PredictMemoryPlan._fields_) == 28
    assert len(_lib.CacheMixPlan._fields_) == 14 and len(_lib.PredictCachePlan._fields_) == 25 and len(_lib.MemoryPlan._fields_) == 12   # unchanged
    lib.jlm_memory_topk_workspace_bytes.restype = ctypes.c_size_t
    lib.jlm_memory_topk_chunk_keys.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t]
    for N, R, K in ((1, 1, 1), (1057, 67, 1024), (10 ** 6, 1024, 64), (1 << 24, 64, 1024)):
        need = lib.jlm_memory_topk_workspace_bytes(N, R, K)
        assert need == fake_memory_topk.TopkLib.jlm_memory_topk_workspace_bytes(N, R, K) == R * (128 + 8 * K)
        for b in (need, need + 4 * R * 32, 4 * M.RetrievalBuffers.workspace_floats(N, R, K), need - 1):
            assert lib.jlm_memory_topk_chunk_keys(N, R, K, b) == fake_memory_topk.TopkLib.jlm_memory_topk_chunk_keys(N, R, K, b)
    assert lib.jlm_memory_topk_workspace_bytes(0, 1, 1) == 0 and lib.jlm_memory_topk_workspace_bytes(5, 1, 1025) == 0
    assert C.MIX_MAX_SIZE >= M.TOPK_MAX                                    # the patch takes a window of K entries
