"""CPU: scoring against a memory of hidden states (jlm_amd/memory.py) -- the float64 definition against a
brute-force loop over an explicit probability vector, and the host path end to end over the numpy double of the new entry points
(tests/fake_memory.py): the five fixture models against the definition over the oracle's own states (OracleLM.lstm_cell), the bits of
the plain -log p, thetas together and apart, the order a memory is built in, concat, save / load, every refusal before a launch, the
command line, the exports."""
import ctypes
import os

import numpy as np
import pytest

from jlm_amd import _lib, cache as C, memory as M
from tests import context_cases as cc
from tests import fake_memory

THETAS = [0.0, 0.5, 2.0]
CUTS = [20, 20, 5]
TOK_ATOL = 1e-5                                  # the suite's bar on a token's -log p (tests/test_gpu_score.py)


@pytest.fixture()
def fake(monkeypatch):
    return fake_memory.install(monkeypatch)


def _model(name):
    cc.set_root(name)
    from jlm_amd.model import LSTM_Model
    return LSTM_Model(experiment_id=1)


def _streams(V, B=3, n=45):
    """-> (memory stream, query stream), each (inputs, targets) [B, n]: the queries draw from a pool of twelve words, the memory's text
    from the first nine of them only -- most queries have a matching entry, a query on one of the other three has none"""
    rng = np.random.RandomState(11)
    pool = rng.choice(np.arange(2, V), size=12, replace=False)
    mem = pool[rng.randint(0, 9, size=(B, n + 1))].astype(np.int32)
    qry = pool[rng.randint(0, 12, size=(B, n + 1))].astype(np.int32)
    return (mem[:, :-1], mem[:, 1:]), (qry[:, :-1], qry[:, 1:])


def _lse(y):
    top = y.max(axis=-1)
    return top + np.log(np.exp(y - top[..., None]).sum(axis=-1))


def oracle_states(name, x, y):
    """-> (h [B, n, H] float64: the state each step leaves, nll [B, n] float64) of streams from the zero state"""
    lm = cc.oracle(name).model
    B, n = x.shape
    h, c = lm.zero_state(B)
    hs, nll = [], []
    sn = lm.config["self_norm"]
    for t in range(n):
        h, c = lm.lstm_cell(x[:, t], h, c)
        yy = np.asarray(lm.project(h), dtype=np.float64)
        yt = yy[np.arange(B), y[:, t]]
        nll.append(-yt if sn else _lse(yy) - yt)
        hs.append(np.array(h, dtype=np.float64))
    return np.stack(hs, axis=1), np.stack(nll, axis=1)


def build_order(a, num_steps):
    """[B, n, ...] -> [B n, ...] in the order Memory.build keeps: (call, t, b)"""
    B, n = a.shape[:2]
    return np.concatenate([np.swapaxes(a[:, lo:lo + num_steps], 0, 1).reshape((-1,) + a.shape[2:]) for lo in range(0, n, num_steps)])


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("theta", [0.0, 0.4, 3.0])
def test_definition_against_explicit_probability_vector(theta):
    rng = np.random.RandomState(5)
    V, N, Q, H = 6, 40, 17, 8
    keys, hq = rng.uniform(-1, 1, size=(N, H)), rng.uniform(-1, 1, size=(Q, H))
    kw, wq = rng.randint(0, V - 1, size=N), rng.randint(0, V, size=Q)              # word V - 1 is never in the memory
    wq[0] = V - 1
    lpm = M.memory_log_probs(hq, wq, keys, kw, [theta, 2 * theta])
    assert lpm.shape == (2, Q)
    for q in range(Q):
        s = np.array([theta * float(np.dot(hq[q], keys[i])) for i in range(N)])
        a = np.exp(s - s.max())
        a /= a.sum()
        p = np.zeros(V)
        for i in range(N):
            p[kw[i]] += a[i]
        assert abs(p.sum() - 1.0) <= 1e-12
        np.testing.assert_allclose(np.exp(lpm[0, q]), p[wq[q]], rtol=0, atol=1e-12)
        assert (lpm[0, q] == -np.inf) == (p[wq[q]] == 0.0)
    assert lpm[0, 0] == -np.inf and np.isfinite(lpm[:, 1:]).any()
    if theta == 0.0:                                                               # counts: log(#matches / N)
        for q in range(1, Q):
            k = int(np.sum(kw == wq[q]))
            assert lpm[0, q] == pytest.approx(np.log(k / N) if k else -np.inf, abs=1e-12)
    for bad in ((hq, wq[:-1], keys, kw), (hq, wq, keys[:0], kw[:0]), (hq[:, :4], wq, keys, kw), (hq, wq, keys, kw[:-1])):
        with pytest.raises(ValueError):
            M.memory_log_probs(*bad, [theta])


# ---------------------------------------------------------------------------------------------- the host path over the double
def _run_cut(m, x, y, memory, spec, cuts, plain=False):
    h = c = hp = cp = None
    parts, at = [], 0
    for k in cuts:
        res = m.score_streams_memory(x[:, at:at + k], y[:, at:at + k], memory, spec, h, c)
        if plain:                                                                  # the same input through score_streams: the same bits
            nll, hp, cp = m.score_streams(x[:, at:at + k], y[:, at:at + k], hp, cp)
            assert nll.tobytes() == res.nll_lm.tobytes() and nll.dtype == res.nll_lm.dtype == np.float64
            assert hp.numpy().tobytes() == res.h.numpy().tobytes() and cp.numpy().tobytes() == res.c.numpy().tobytes()
        assert res.nll(0).tobytes() == res.nll_lm.tobytes() and res.n_entries == memory.N
        h, c = res.h, res.c
        parts.append(res)
        at += k
    assert at == x.shape[1]
    return np.concatenate([p.nll_lm for p in parts], axis=1), np.concatenate([p.logp_memory for p in parts], axis=2)


def _bars(dev_q, ora_q, dev_k, ora_k, want, thetas):
    """[n_theta, Q]: what the difference between the double's states (float32, split rows quantised) and the oracle's can move an
    lpm -- log sum exp is 1-Lipschitz in the largest |delta s_i|, once for log M and once for log Z -- plus the float32 result's
    rounding; 0 where the definition is exact (-inf)"""
    dq, dk = dev_q - ora_q, dev_k - ora_k
    move = (np.abs(ora_k @ dq.T) + np.abs(dk @ ora_q.T) + np.abs(dk @ dq.T)).max(axis=0)            # [Q]
    out = np.zeros_like(want)
    for t, theta in enumerate(thetas):
        out[t] = 2 * theta * move + 2.0 ** -23 * (1 + np.abs(np.where(np.isfinite(want[t]), want[t], 0.0)))
    return np.where(np.isfinite(want), out, 0.0)


@pytest.mark.parametrize("name", list(cc.MODELS))
def test_streams_and_sequences_match_the_definition(name, fake):
    m = _model(name)
    V, H = cc.MODELS[name][:2]
    (xm, ym), (xq, yq) = _streams(V)
    B, n = xq.shape
    ora_k, _nll = oracle_states(name, xm, ym)
    ora_q, ora_nll = oracle_states(name, xq, yq)
    ora_k, ora_q_flat = build_order(ora_k, 20), ora_q.reshape(B * n, H)
    want = M.memory_log_probs(ora_q_flat, yq.reshape(-1), ora_k, build_order(ym, 20), THETAS)          # [n_theta, B n]
    # the condition of this test, from the float64 definition alone: most queries have a matching entry and some have none
    has = np.isfinite(want[0])
    assert has.mean() >= 0.5 and (~has).any(), (name, float(has.mean()))

    memory = M.Memory.build(m, xm, ym, 20)
    assert memory.N == len(memory) == B * n and (memory.H, memory.V) == (H, V) and memory.nbytes == B * n * (4 * H + 4)
    dev_k, dev_w = memory.numpy()
    assert dev_k.dtype == np.float32 and dev_k.shape == (B * n, H) and dev_w.dtype == np.int64
    assert np.array_equal(dev_w, build_order(ym, 20))                                                  # the order (call, t, b)
    np.testing.assert_allclose(dev_k, ora_k, rtol=0, atol=1e-4)
    dev_q = M.Memory.build(m, xq, yq, n).numpy()[0].astype(np.float64).reshape(n, B, H).transpose(1, 0, 2).reshape(B * n, H)

    spec = M.MemorySpec(theta=THETAS, lam=0.2)
    nll, lpm = _run_cut(m, xq, yq, memory, spec, CUTS, plain=True)
    assert lpm.shape == (3, B, n) and nll.shape == (B, n) and lpm.dtype == np.float64
    np.testing.assert_allclose(nll, ora_nll, rtol=0, atol=TOK_ATOL)
    got = lpm.reshape(3, B * n)
    bars = _bars(dev_q, ora_q_flat, dev_k.astype(np.float64), ora_k, want, THETAS)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and not np.isnan(got).any()
    err = np.abs(got[:, has] - want[:, has])
    print("%s: max |lpm - definition| %.3e, max err / bar %.3f" % (name, err.max(), (err / bars[:, has]).max()))
    assert np.all(err <= bars[:, has])
    # the mixture: cache.mix_nll with n_entries = N over the oracle's numbers
    for t in (0, 2):
        mixed = np.concatenate([p for p in [_run_cut(m, xq, yq, memory, spec, [n])[0]]])              # (one call: the same nll)
        np.testing.assert_allclose(mixed, nll, rtol=0, atol=1e-9)
        res = m.score_streams_memory(xq, yq, memory, spec)
        want_mix = C.mix_nll(ora_nll.reshape(-1), want[t], memory.N, 0.2).reshape(B, n)
        assert np.all(np.abs(res.nll(0.2, t) - want_mix) <= TOK_ATOL + bars[t].reshape(B, n))
        miss = ~has.reshape(B, n)
        np.testing.assert_allclose(res.nll(0.2, t)[miss], res.nll_lm[miss] - np.log1p(-0.2), rtol=0, atol=1e-12)
    # every query sees every entry: another cut of the stream gives the same lpm (the double sums in float64)
    nll2, lpm2 = _run_cut(m, xq, yq, memory, spec, [7, 38])
    fin = np.isfinite(lpm)
    assert np.array_equal(np.isfinite(lpm2), fin)
    np.testing.assert_allclose(lpm2[fin], lpm[fin], rtol=0, atol=2e-6)
    # three thetas in one call are three calls
    for t, theta in enumerate(THETAS):
        one = m.score_streams_memory(xq, yq, memory, M.MemorySpec(theta=theta))
        assert one.logp_memory.shape == (1, B, n) and one.logp_memory[0].tobytes() == res.logp_memory[t].tobytes()
    # sentence mode: every row of score_memory is the stream call of that sequence alone
    seqs = [[int(w) for w in yq[0, :L]] for L in (9, 0, 30, 1, 17, 0, 30)]
    one_spec = M.MemorySpec(theta=0.5, lam=0.25)
    rows = m.score_memory(seqs, cc.EOS, memory, one_spec)
    assert [len(g) for g in rows] == [len(s) for s in seqs] and all(g.dtype == np.float64 for g in rows)
    for s, g in zip(seqs, rows):
        if len(s):
            alone = m.score_streams_memory(np.array([[cc.EOS] + s[:-1]]), np.array([s]), memory, one_spec)
            np.testing.assert_allclose(g, alone.nll(0.25)[0], rtol=0, atol=1e-6)
            xs = np.array([[cc.EOS] + s[:-1]])
            oh, onll = oracle_states(name, xs, np.array([s]))
            w1 = M.memory_log_probs(oh[0], s, ora_k, build_order(ym, 20), [0.5])
            dq = M.Memory.build(m, xs, np.array([s]), len(s)).numpy()[0].astype(np.float64)
            bar = TOK_ATOL + _bars(dq, oh[0], dev_k.astype(np.float64), ora_k, w1, [0.5])[0]
            assert np.all(np.abs(g - C.mix_nll(onll[0], w1[0], memory.N, 0.25)) <= bar)
    for max_rows in (1, 2):
        again = m.score_memory(seqs, cc.EOS, memory, one_spec, max_rows=max_rows)
        assert all(np.allclose(a, b, rtol=0, atol=1e-6) for a, b in zip(rows, again))
    assert m.score_memory([], cc.EOS, memory, one_spec) == []


def test_build_order_concat_and_calls(fake):
    m = _model("tied")
    (xm, ym), (xq, yq) = _streams(cc.MODELS["tied"][0])
    B, n = xm.shape
    a = M.Memory.build(m, xm, ym, 20)
    whole = M.Memory.build(m, xm, ym, n)
    # calls follow one another in time, so (call, t, b) is (t, b) whatever num_steps: entry t B + b is step t of stream b
    assert np.array_equal(whole.numpy()[1], ym.T.reshape(-1)) and np.array_equal(a.numpy()[1], build_order(ym, 20))
    assert np.array_equal(a.numpy()[1], whole.numpy()[1]) and np.array_equal(M.Memory.build(m, xm, ym, 1).numpy()[1], whole.numpy()[1])
    np.testing.assert_allclose(a.numpy()[0], whole.numpy()[0], rtol=0, atol=1e-6)          # the state carried across calls
    assert not np.array_equal(whole.numpy()[1], ym.reshape(-1))                             # ... and not stream after stream
    b = M.Memory.build(m, xq[:2], yq[:2], 20)
    both = M.Memory.concat(a, b)
    assert both.N == a.N + b.N == B * n + 2 * n
    assert both.keys[:a.N].numpy().tobytes() == a.keys.numpy().tobytes() and both.keys[a.N:].numpy().tobytes() == b.keys.numpy().tobytes()
    assert np.array_equal(both.numpy()[1], np.concatenate([a.numpy()[1], b.numpy()[1]]))
    spec = M.MemorySpec(theta=[0.5])
    ra, rboth = m.score_streams_memory(xq, yq, a, spec), m.score_streams_memory(xq, yq, both, spec)
    assert ra.nll_lm.tobytes() == rboth.nll_lm.tobytes()
    # more entries: a query that had a match keeps one; the queries' own text is in `both`, so rows 0 and 1 match everywhere
    assert np.all(np.isfinite(rboth.logp_memory[0][np.isfinite(ra.logp_memory[0])])) and np.isfinite(rboth.logp_memory[0, :2]).all()
    other = _model("untied")
    with pytest.raises(ValueError):
        M.Memory.concat(a, M.Memory.build(other, xm, ym, 20))
    with pytest.raises(ValueError):
        M.Memory.concat(a, None)


def test_save_load_round_trip_and_refusals(fake, tmp_path):
    m = _model("tied")
    (xm, ym), (xq, yq) = _streams(cc.MODELS["tied"][0])
    mem = M.Memory.build(m, xm, ym, 20)
    path = str(tmp_path / "mem.npz")
    mem.save(path)
    back = M.Memory.load(m, path)
    assert back.N == mem.N and (back.H, back.split, back.h_scale, back.V) == (mem.H, mem.split, mem.h_scale, mem.V)
    assert back.keys.numpy().tobytes() == mem.keys.numpy().tobytes() and back.words.numpy().tobytes() == mem.words.numpy().tobytes()
    spec = M.MemorySpec(theta=[0.0, 0.7])
    assert m.score_streams_memory(xq, yq, back, spec).logp_memory.tobytes() == m.score_streams_memory(xq, yq, mem, spec).logp_memory.tobytes()
    with np.load(path) as z:
        fields = {k: z[k] for k in z.files}
    assert sorted(fields) == ["H", "V", "h_scale", "keys", "split", "words"]
    del fake.launches[:]
    for k, v in (("H", mem.H * 2), ("split", 1 - int(mem.split)), ("h_scale", mem.h_scale * 2), ("V", mem.V + 1)):
        bad = str(tmp_path / ("bad_%s.npz" % k))
        np.savez(bad, **dict(fields, **{k: np.asarray(v, dtype=fields[k].dtype)}))
        with pytest.raises(ValueError, match=k):
            M.Memory.load(m, bad)
    for k in fields:                                                               # a file without one of the six
        bad = str(tmp_path / ("no_%s.npz" % k))
        np.savez(bad, **{j: v for j, v in fields.items() if j != k})
        with pytest.raises(ValueError):
            M.Memory.load(m, bad)
    for k, v in (("keys", fields["keys"].astype(np.float64)), ("keys", fields["keys"][:, :32]), ("words", fields["words"][:-1]),
                 ("words", fields["words"].astype(np.int64)), ("keys", fields["keys"][:0])):
        bad = str(tmp_path / "bad_shape.npz")
        np.savez(bad, **dict(fields, **{k: v, "words": fields["words"][:0] if len(v) == 0 else (v if k == "words" else fields["words"])}))
        with pytest.raises(ValueError):
            M.Memory.load(m, bad)
    # a model of another shape refuses it whole
    with pytest.raises(ValueError):
        M.Memory.load(_model("tied-h512"), path)
    assert fake.launches == []


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(theta=-0.1), dict(theta=float("nan")), dict(theta=float("inf")), dict(theta=[]), dict(theta=[0.1] * 17),
                                dict(theta=[0.1, -1]), dict(theta="x"), dict(theta=True), dict(lam=1.0), dict(lam=-0.01),
                                dict(lam=float("nan")), dict(lam=None), dict(lam=True)])
def test_spec_refuses(kw):
    with pytest.raises(ValueError):
        M.MemorySpec(**kw)


def test_spec_accepts():
    s = M.MemorySpec()
    assert (s.thetas, s.theta, s.lam) == ((0.3,), 0.3, 0.1)
    s = M.MemorySpec(theta=[0, 0.5], lam=0)
    assert (s.thetas, s.theta, s.lam) == ((0.0, 0.5), 0.0, 0.0)
    assert len(M.MemorySpec(np.linspace(0, 1, 16)).thetas) == 16
    assert M.MAX_KEYS == 1 << 24
    for N in (1, 511, 512, 513, 65536, 65537, 10 ** 5, 10 ** 6, 1 << 24):
        S = M.keys_per_split(N)
        assert S == fake_memory.keys_per_split(N) and S >= 512 and S % 64 == 0 and -(-N // S) <= 128


def test_a_model_with_f32_rows_has_no_scale_field():
    """a DeviceModel without split rows carries no h_scale: the memory's format field is 1 (the launcher does not read it)"""
    import torch

    class F32Rows:
        H, V, split_lstm = 32, 10, False

    mem = M.Memory(F32Rows(), torch.zeros(3, 32), torch.zeros(3, dtype=torch.int32))
    assert (mem.H, mem.split, mem.h_scale, mem.V, mem.N) == (32, False, 1.0, 10, 3)
    with pytest.raises(ValueError):
        M.Memory(F32Rows(), torch.zeros(3, 64), torch.zeros(3, dtype=torch.int32))


def test_refusals_launch_nothing(fake):
    import torch
    m = _model("tied")
    other = _model("untied")
    V = cc.MODELS["tied"][0]
    (xm, ym), (xq, yq) = _streams(V, n=6)
    spec = M.MemorySpec()
    mem = M.Memory.build(m, xm, ym, 6)
    foreign = M.Memory.build(other, xm, ym, 6)
    ok = m.score_streams_memory(xq, yq, mem, spec)
    del fake.launches[:]
    bad_y = yq.copy()
    bad_y[1, 2] = V
    for a, kw in (((xq, yq[:, :5], mem, spec), {}), ((xq[0], yq[0], mem, spec), {}), ((xq, bad_y, mem, spec), {}), ((-xq, yq, mem, spec), {}),
                  ((xq, yq, mem, None), {}), ((xq, yq, mem, (0.3, 0.1)), {}), ((xq, yq, mem, C.CacheSpec(4)), {}), ((xq, yq, None, spec), {}),
                  ((xq, yq, foreign, spec), {}), ((xq, yq, mem, spec), dict(h=ok.h)),
                  ((xq, yq, mem, spec), dict(h=torch.zeros(2, 64), c=torch.zeros(2, 64)))):
        with pytest.raises(ValueError):
            m.score_streams_memory(*a, **kw)
    for kw in (dict(sequences=[[1, V]]), dict(start=-1), dict(spec=None), dict(memory=foreign), dict(memory=None), dict(max_rows=0)):
        args = dict(sequences=[[2, 3]], start=cc.EOS, memory=mem, spec=spec)
        args.update(kw)
        with pytest.raises(ValueError):
            m.score_memory(**args)
    for a in ((xm, ym[:, :5]), (xm, bad_y), (xm[:, :0], ym[:, :0]), (xm[:0], ym[:0])):
        with pytest.raises(ValueError):
            M.Memory.build(m, *a)
    for steps in (0, -1, 2.0, None, True):
        with pytest.raises(ValueError):
            M.Memory.build(m, xm, ym, steps)
    with pytest.raises(ValueError):
        ok.nll(0.1, 1)
    with pytest.raises(ValueError):
        ok.nll(1.0)
    assert fake.launches == []
    empty = m.score_streams_memory(xq[:, :0], yq[:, :0], mem, M.MemorySpec([0.1, 0.2]), ok.h, ok.c)
    assert empty.nll_lm.shape == (3, 0) and empty.logp_memory.shape == (2, 3, 0) and empty.h is ok.h and empty.c is ok.c
    assert [len(g) for g in m.score_memory([[], []], cc.EOS, mem, spec)] == [0, 0]
    assert fake.launches == []
    m.score_streams_memory(xq, yq, mem, spec)
    assert fake.launches == ["score_memory_frames", "memory_rows"]


def test_flagged_product_raises(fake):
    import torch
    m = _model("tied")
    (xm, ym), (xq, yq) = _streams(cc.MODELS["tied"][0], n=6)
    mem = M.Memory.build(m, xm, ym, 6)
    keys = mem.keys.clone()
    keys.view(torch.int32)[4, 3] = 0x7fc00000 if not mem.split else 0x7e007e00                 # a NaN in either row format
    with pytest.raises(_lib.JlmHipError, match="not finite"):
        m.score_streams_memory(xq, yq, M.Memory(m.dev, keys, mem.words), M.MemorySpec())


def test_launcher_refusals(fake):
    """the header's refusals of jlm_memory_rows, each -1 with nothing launched; empty shapes return 0 with nothing launched"""
    import torch
    rng = np.random.RandomState(0)
    N, H, R, S = 40, 32, 2, 4
    keys = torch.from_numpy(rng.uniform(-1, 1, size=(N, H)).astype(np.float32))
    q_rows = torch.from_numpy(rng.uniform(-1, 1, size=(S, R, H)).astype(np.float32))
    kw, qw = torch.zeros(N, dtype=torch.int32), torch.zeros((S, R), dtype=torch.int32)
    length = torch.full((R,), S, dtype=torch.int32)
    lpm = torch.full((1, S, R), 5.0)
    lib = _lib.lib()
    need = lib.jlm_memory_workspace_bytes(N, R, S, 1)
    assert need == 1 * 1 * 3 * R * S * 4 and lib.jlm_memory_workspace_bytes(1100, R, S, 3) == 3 * 3 * 3 * R * S * 4
    assert lib.jlm_memory_workspace_bytes(0, R, S, 1) == 0 and lib.jlm_memory_keys_per_split(10 ** 6) == 7872
    ws = torch.zeros(need // 4)
    th = (ctypes.c_float * 17)(*([0.5] * 17))
    neg = (ctypes.c_float * 1)(-1.0)
    nan = (ctypes.c_float * 1)(float("nan"))
    base = dict(keys=keys.data_ptr(), key_words=kw.data_ptr(), N=N, H=H, split=0, h_scale=1.0, q_rows=q_rows.data_ptr(), q_words=qw.data_ptr(),
                n_rows=R, n_steps=S, length=length.data_ptr(), thetas=th, n_theta=1, lpm=lpm.data_ptr(), workspace=ws.data_ptr(),
                workspace_bytes=need, flags=None, stream=0)
    call = lambda **k: lib.jlm_memory_rows(**dict(base, **k))
    del fake.launches[:]
    for k in (dict(N=0), dict(N=-1), dict(N=(1 << 24) + 1), dict(H=0), dict(H=48), dict(H=-32), dict(keys=keys.data_ptr() + 4),
              dict(q_rows=q_rows.data_ptr() + 8), dict(key_words=kw.data_ptr() + 2), dict(q_words=qw.data_ptr() + 1), dict(keys=None),
              dict(key_words=None), dict(q_rows=None), dict(q_words=None), dict(lpm=None), dict(workspace=None), dict(lpm=lpm.data_ptr() + 2),
              dict(length=length.data_ptr() + 2), dict(n_theta=0), dict(n_theta=17), dict(thetas=None), dict(thetas=neg), dict(thetas=nan),
              dict(split=1, h_scale=0.0), dict(split=1, h_scale=-1.0), dict(n_rows=-1), dict(n_steps=-1), dict(n_rows=65536),
              dict(workspace_bytes=need - 4), dict(n_theta=2)):
        assert call(**k) == -1, k
    assert call(n_rows=0) == 0 and call(n_steps=0) == 0
    assert fake.launches == [] and bool((lpm == 5.0).all())
    assert call(length=None) == 0 and fake.launches == ["memory_rows"] and not bool((lpm == 5.0).any())


# ---------------------------------------------------------------------------------------------- the command line
def _write(root, name, lines):
    with open(os.path.join(root, "data", name), "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return os.path.join(root, "data", name)


def test_command_line(fake, capsys, tmp_path):
    from jlm_amd import perplexity
    from jlm_amd.data import Vocab
    lines_of = lambda: [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("LSTM model:")]     # (the loader's own line)
    root = cc.model_root("tied")
    cc.set_root("tied")
    os.makedirs(os.path.join(root, "data"), exist_ok=True)
    vocab = Vocab(cc.MODELS["tied"][0])
    words = [w for w in vocab.t2i if w not in ("<unk>", "<eos>")]
    rng = np.random.RandomState(8)
    passage = " ".join(words[i] for i in rng.choice(len(words), size=29, replace=False))
    text = _write(root, "memory_text.txt", [passage] * 12)
    test = _write(root, "memory_test.txt", [passage] * 8)
    dev = _write(root, "memory_dev.txt", [passage] * 6)
    mem_path = str(tmp_path / "mem.npz")
    model_args = ["--root", root, "-e", "1"]
    built = M.main(model_args + ["--text", text, "-b", "2", "--num_steps", "10", "--out", mem_path])
    out = lines_of()
    assert built.N == 2 * 170 and out == ["memory: N 340  H 64  bytes {}  -> {}".format(340 * (4 * 64 + 4), mem_path)]
    common = model_args + ["--mode", "stream", "-b", "2", "--num_steps", "10", "--file", test]
    # without --memory: the plain path (LSTM_Model.score_streams through stream_perplexity) is what runs, and prints what it printed
    calls = []
    keep = perplexity.stream_perplexity
    perplexity.stream_perplexity = lambda *a: calls.append(a[2:]) or (7.5, 1.0, 10)
    try:
        assert perplexity.main(common) == 7.5
    finally:
        perplexity.stream_perplexity = keep
    out = lines_of()
    assert calls == [(2, 10)] and len(out) == 2 and out[0].startswith("tokens: 10  <unk>: 0  tokens/s: ") and out[1] == "Test perplexity: 7.5"
    del fake.launches[:]
    plain = perplexity.main(common)
    out_plain = lines_of()
    assert len(out_plain) == 2 and out_plain[1] == "Test perplexity: {}".format(plain) and "score_memory_frames" not in fake.launches
    # with --memory: the same plain perplexity, then a lower one under the memory of the same passage
    pp = perplexity.main(common + ["--memory", mem_path, "--mem-theta", "0.5", "--mem-lam", "0.2"])
    out = lines_of()
    assert pp == plain and len(out) == 3 and out[1] == out_plain[1] and out[0].split("  tokens/s")[0] == out_plain[0].split("  tokens/s")[0]
    assert out[2].startswith("Test perplexity with memory (N 340 theta 0.5 lam 0.2): ") and float(out[2].rsplit(" ", 1)[1]) < pp
    pp2 = perplexity.main(common + ["--memory", mem_path, "--tune-memory", dev, "--thetas", "0,0.5,2", "--lams", "0,0.2,0.6"])
    out = lines_of()
    assert pp2 == plain and len(out) == 4 and out[2].startswith("Memory tuned on {}: theta ".format(dev))
    assert out[3].startswith("Test perplexity with memory (N 340 theta ") and float(out[3].rsplit(" ", 1)[1]) < pp
    ng = _write(root, "memory_unused.arpa", ["\\data\\"])
    for bad in (["--memory", mem_path, "--cache", "8"], ["--memory", mem_path, "--dynamic"], ["--memory", mem_path, "--ngram", ng],
                ["--memory", mem_path, "--mode", "sentence"], ["--memory", mem_path, "--mem-lam", "1"], ["--memory", mem_path, "--mem-theta", "-1"],
                ["--memory", mem_path, "--tune-memory", dev, "--lams", "0,2"], ["--tune-memory", dev],
                ["--memory", str(tmp_path / "missing.npz")]):
        with pytest.raises(SystemExit):
            perplexity.main(common + bad)
    capsys.readouterr()


# ---------------------------------------------------------------------------------------------- the exports
def test_lib_exposes_the_memory_entries():
    names = ("jlm_memory_rows", "jlm_memory_workspace_bytes", "jlm_memory_keys_per_split", "jlm_score_memory_frames")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(n in _lib.EXPORTS and hasattr(lib, n) for n in names)
    assert [f[0] for f in _lib.MemoryPlan._fields_] == ["keys", "key_words", "N", "q_rows", "q_words", "len", "thetas", "n_theta", "lpm",
                                                        "workspace", "workspace_bytes", "flags"]
    assert len(_lib.ScorePlan._fields_) == 18 and len(_lib.CachePlan._fields_) == 11                  # unchanged
    # the split size is the header's function of N alone, in the library as in the package
    lib.jlm_memory_keys_per_split.restype = ctypes.c_int
    lib.jlm_memory_workspace_bytes.restype = ctypes.c_size_t
    for N in (1, 511, 512, 513, 1057, 65536, 65537, 10 ** 5, 10 ** 6, 1 << 24):
        S = lib.jlm_memory_keys_per_split(N)
        assert S == M.keys_per_split(N)
        assert lib.jlm_memory_workspace_bytes(N, 3, 7, 2) == 2 * (-(-N // S)) * 3 * 21 * 4
    assert lib.jlm_memory_keys_per_split(0) == 0 and lib.jlm_memory_keys_per_split((1 << 24) + 1) == 0
