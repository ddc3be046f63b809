"""GPU: scoring against a memory of hidden states end to end (LSTM_Model.score_streams_memory / score_memory, Memory.build / save /
load; csrc jlm_score_memory_frames + memory_rows_kernel + memory_fold_kernel) against the float64 definition
(jlm_amd.memory.memory_log_probs) over the oracle's own states (OracleLM.lstm_cell, oracle/jlm_oracle.py): the cases of
tests/test_memory_cpu.py on the device, on the five models of tests/test_gpu_cache.py.

The bar of a position is computed here from what the device returned, not a constant: the kernel's derived bar
(tests/memory_budget.py; derivation in tests/test_gpu_memory_rows.py) plus what the difference D between the device's states and the
oracle's can move a score, theta (|Dq . k| + |q . Dk| + |Dq . Dk|), maximised over the memory -- exactly as tests/test_gpu_cache.py
widens its own.  The device's states are Memory.numpy() of memories built from the two texts.  nll_lm and the returned state must be
score_streams' bits."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import cache as C, memory as M                                                 # noqa: E402
from tests.gpu_rows import UNTIED_F32, fixture_model, oracle_lm                             # noqa: E402
from tests.memory_budget import kernel_bar                                                  # noqa: E402
from tests.test_gpu_cache import oracle_states                                              # noqa: E402

pytestmark = pytest.mark.gpu

MODELS = ["small-tied", "small-vtable", "small-tied-sn", "odd-tied", UNTIED_F32]
THETAS = [0.0, 0.5, 2.0]
CUTS = [20, 20, 5]
TOK_ATOL = 1e-5                                                                              # tests/test_gpu_score.py's bar on nll


def _streams(V, B=3, n=45):
    """tests/test_memory_cpu.py's texts: the queries over a pool of twelve words, the memory's text over the first nine of them"""
    rng = np.random.RandomState(11)
    pool = rng.choice(np.arange(2, V), size=12, replace=False)
    mem = pool[rng.randint(0, 9, size=(B, n + 1))].astype(np.int32)
    qry = pool[rng.randint(0, 12, size=(B, n + 1))].astype(np.int32)
    return (mem[:, :-1], mem[:, 1:]), (qry[:, :-1], qry[:, 1:])


def tb(a):
    """[B, n, ...] -> [n B, ...]: the order Memory.build keeps, (t, b)"""
    return np.swapaxes(a, 0, 1).reshape((-1,) + a.shape[2:])


def bars(dev_q, ora_q, dev_k, ora_k, q_words, k_words, thetas, split):
    """[n_theta, Q]: kernel_bar over the device's operands plus theta (|Dq.k| + |q.Dk| + |Dq.Dk|) maximised over the memory; 0 where the
    definition is exact (-inf)"""
    N, H = ora_k.shape
    dk = dev_k - ora_k
    out = np.zeros((len(thetas), len(q_words)))
    for q in range(len(q_words)):
        same = k_words == q_words[q]
        if not same.any():
            continue
        dq = dev_q[q] - ora_q[q]
        move = float((np.abs(ora_k @ dq) + np.abs(dk @ ora_q[q]) + np.abs(dk @ dq)).max())
        A = float((np.abs(dev_k) @ np.abs(dev_q[q])).max())
        dot = ora_k @ ora_q[q]
        for t, theta in enumerate(thetas):
            s = theta * dot
            m = s.max()
            logZ, logM = np.log(np.exp(s - m).sum()), np.log(np.exp(s[same] - m).sum())
            out[t, q] = kernel_bar(split, H, N, theta, A, logM, logZ) + theta * move
    return out


def _run_cut(model, x, y, memory, spec, cuts):
    """the stream in calls of ``cuts`` steps, state carried; every call against score_streams on the same input: the same bits"""
    h = c = hp = cp = None
    parts, at = [], 0
    for k in cuts:
        res = model.score_streams_memory(x[:, at:at + k], y[:, at:at + k], memory, spec, h, c)
        nll, hp, cp = model.score_streams(x[:, at:at + k], y[:, at:at + k], hp, cp)
        assert nll.tobytes() == res.nll_lm.tobytes() and nll.dtype == res.nll_lm.dtype == np.float64
        assert torch.equal(hp.view(torch.int32), res.h.view(torch.int32)) and torch.equal(cp, res.c)
        assert res.nll(0).tobytes() == res.nll_lm.tobytes() and res.n_entries == memory.N
        h, c = res.h, res.c
        parts.append(res)
        at += k
    return np.concatenate([p.nll_lm for p in parts], axis=1), np.concatenate([p.logp_memory for p in parts], axis=2)


@pytest.mark.parametrize("name", MODELS)
def test_streams_match_the_definition(name, fx, monkeypatch, tmp_path):
    f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    lm = oracle_lm(f["root"])
    (xm, ym), (xq, yq) = _streams(m.V)
    B, n = xq.shape
    ora_k, _nll = oracle_states(lm, xm, ym)
    ora_q, ora_nll = oracle_states(lm, xq, yq)
    ora_k, ora_qf, k_words, q_words = tb(ora_k), tb(ora_q), tb(ym), tb(yq)
    want = M.memory_log_probs(ora_qf, q_words, ora_k, k_words, THETAS)                       # [n_theta, n B], order (t, b)
    has = np.isfinite(want[0])
    assert has.mean() >= 0.5 and (~has).any()                                                # matches and misses, by the definition alone

    memory = M.Memory.build(model, xm, ym, 20)
    dev_k, dev_w = memory.numpy()
    assert memory.N == B * n and np.array_equal(dev_w, k_words) and dev_k.shape == (B * n, m.H)
    dev_k = dev_k.astype(np.float64)
    dev_q = M.Memory.build(model, xq, yq, n).numpy()[0].astype(np.float64)
    print("%s: max |k_dev - k_oracle| %.3e, max |q_dev - q_oracle| %.3e" % (name, np.abs(dev_k - ora_k).max(), np.abs(dev_q - ora_qf).max()))

    spec = M.MemorySpec(theta=THETAS, lam=0.2)
    nll, lpm = _run_cut(model, xq, yq, memory, spec, CUTS)
    np.testing.assert_allclose(nll, ora_nll, rtol=0, atol=TOK_ATOL)
    got = tb(lpm.transpose(1, 2, 0)).T                                                       # [n_theta, n B]
    bar = bars(dev_q, ora_qf, dev_k, ora_k, q_words, k_words, THETAS, bool(m.split_lstm))
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and not np.isnan(got).any()
    err = np.abs(got[:, has] - want[:, has])
    print("%s: %d finite lpm, max err / bar %.3f, largest bar %.3e" % (name, int(has.sum()) * 3, float((err / bar[:, has]).max()), bar.max()))
    assert np.all(err <= bar[:, has]), (name, float(err.max()))
    # the mixture: mix_nll with n_entries = N; logaddexp is 1-Lipschitz in the larger of its arguments' errors
    whole = model.score_streams_memory(xq, yq, memory, spec)
    for t in range(3):
        want_mix = C.mix_nll(tb(ora_nll), want[t], memory.N, 0.2)
        assert np.all(np.abs(tb(whole.nll(0.2, t)) - want_mix) <= TOK_ATOL + bar[t])
    # every query sees every entry: another cut of the stream gives the same lpm -- within the kernel's part of the bar (D = 0) for
    # certain, and bit for bit whenever the two cuts left the same state bits (a query's bits do not depend on the call's shape:
    # tests/test_gpu_memory_rows.py)
    kb = bars(dev_q, dev_q, dev_k, dev_k, q_words, k_words, THETAS, bool(m.split_lstm))
    wl = tb(whole.logp_memory.transpose(1, 2, 0)).T
    assert np.array_equal(np.isneginf(wl), np.isneginf(got)) and np.all(np.abs(wl[:, has] - got[:, has]) <= 2 * kb[:, has])
    print("%s: one call against %s: lpm bit-equal: %s" % (name, CUTS, whole.logp_memory.tobytes() == lpm.tobytes()))
    for t, theta in enumerate(THETAS):                                                       # three thetas in one call are three calls
        one = model.score_streams_memory(xq, yq, memory, M.MemorySpec(theta=theta))
        assert one.logp_memory[0].tobytes() == whole.logp_memory[t].tobytes()
    # a memory that was saved and reloaded gives the same bits
    path = str(tmp_path / "mem.npz")
    memory.save(path)
    back = M.Memory.load(model, path)
    assert torch.equal(back.keys.view(torch.int32), memory.keys.view(torch.int32)) and torch.equal(back.words, memory.words)
    assert model.score_streams_memory(xq, yq, back, spec).logp_memory.tobytes() == whole.logp_memory.tobytes()
    both = M.Memory.concat(memory, back)
    assert both.N == 2 * memory.N and np.array_equal(np.isneginf(model.score_streams_memory(xq, yq, both, spec).logp_memory), np.isneginf(lpm))


@pytest.mark.parametrize("name", ["small-tied", UNTIED_F32])
def test_score_memory_ragged_sequences(name, fx, monkeypatch):
    """ragged sequences, empty ones included: the mixed -log p against the definition over the oracle's states and -log p, and,
    chunked by max_rows, equal to the unchunked result row by row -- bit for bit: a query's lpm does not depend on its call"""
    f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    lm = oracle_lm(f["root"])
    (xm, ym), (_xq, yq) = _streams(m.V)
    memory = M.Memory.build(model, xm, ym, 20)
    ora_k = tb(oracle_states(lm, xm, ym)[0])
    dev_k = memory.numpy()[0].astype(np.float64)
    seqs = [[int(w) for w in yq[i % 3, :L]] for i, L in enumerate((9, 0, 30, 1, 17, 0, 30))]
    spec = M.MemorySpec(theta=0.7, lam=0.25)
    got = model.score_memory(seqs, 1, memory, spec)
    assert [len(g) for g in got] == [len(s) for s in seqs] and all(g.dtype == np.float64 for g in got)
    for s, g in zip(seqs, got):
        if not len(s):
            continue
        x, y = np.array([[1] + s[:-1]]), np.array([s])
        ora_h, ora_nll = oracle_states(lm, x, y)
        dev_q = M.Memory.build(model, x, y, len(s)).numpy()[0].astype(np.float64)
        want_lpm = M.memory_log_probs(ora_h[0], y[0], ora_k, tb(ym), spec.thetas)
        want = C.mix_nll(ora_nll[0], want_lpm[0], memory.N, spec.lam)
        bar = TOK_ATOL + bars(dev_q, ora_h[0], dev_k, ora_k, y[0], tb(ym), spec.thetas, bool(m.split_lstm))[0]
        assert np.all(np.abs(g - want) <= bar), (name, len(s), float(np.abs(g - want).max()))
    for max_rows in (1, 2):
        again = model.score_memory(seqs, 1, memory, spec, max_rows=max_rows)
        plain = model.score(seqs, 1, max_rows=max_rows)
        lam0 = model.score_memory(seqs, 1, memory, M.MemorySpec(theta=0.7, lam=0.0), max_rows=max_rows)
        assert all(a.tobytes() == p.tobytes() for a, p in zip(lam0, plain))                  # lam = 0: score()'s bits in the same row plan
        # the plain -log p of a row may differ between row plans within its bar; the memory's term does not differ at all
        assert all(np.allclose(a, b, rtol=0, atol=2 * TOK_ATOL) for a, b in zip(again, got))


def test_memory_of_another_model_is_refused(fx, monkeypatch):
    _f, model = fixture_model(fx, "small-tied", monkeypatch)
    _f2, other = fixture_model(fx, "small-vtable", monkeypatch)
    (xm, ym), (xq, yq) = _streams(model.dev.V, n=6)
    memory = M.Memory.build(model, xm, ym, 6)
    with pytest.raises(ValueError, match="of this model"):
        other.score_streams_memory(xq, yq, memory, M.MemorySpec())
    with pytest.raises(ValueError):
        model.score_streams_memory(xq, yq, memory, C.CacheSpec(4))
