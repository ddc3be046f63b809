"""CPU: the continuous cache in decode -- the yardstick checks itself (tests/decode_cache_cases.py), the host
plan of ``prime(cache=)``, every refusal, and the host-side search under the cache against the proxy."""
import types

import numpy as np
import pytest

from jlm_amd import config as jconfig, context as jctx
from jlm_amd.cache import CacheSpec
from tests import context_cases as cc
from tests import decode_cache_cases as dc
from tests import fake_hip
from tests.decode_cache_budget import word_bar


# ---------------------------------------------------------------------------------------------- the yardstick checks itself
@pytest.mark.parametrize("name", ["tied", "vtable", "tied-h512"])
def test_cached_oracle_is_the_chain_rule_and_moves_the_result(name):
    """the proxy's 1-best score = the chain-rule sum of -log p_mix along its path, to 1e-9; with the chosen theta and lambda the cached
    oracle's 1-best differs from the primed oracle's on at least 4 of the 12 inputs, and on every input with context words the two top
    scores differ by more than twice the GPU test's bar -- the fixture cannot degenerate silently"""
    o = dc.oracle(name)
    H = cc.MODELS[name][1]
    moved = 0
    for N in dc.SIZES:
        for text, ctx in zip(dc.sentences(), dc.contexts(name)):
            got = dc.cached_decode(o, text, ctx, N, beam_width=5)
            score, words = got[0]
            want = dc.chain_nll_mix(o.model, [cc.EOS] + cc.ids_of(ctx), cc.path_ids(o, words), N).sum()
            assert abs(score - want) <= 1e-9, (name, N, text, score, want)
            primed = cc.primed_decode(o, text, ctx, beam_width=5)
            if not cc.ids_of(ctx):
                assert got == primed                                        # an empty window: the primed oracle's own decode
                continue
            moved += (N == 16) and got[0][1] != primed[0][1]
            bar = 2e-5 + 2e-6 * abs(score) + word_bar(True, H, N, dc.THETA) * max(len(words), 1)
            assert abs(score - primed[0][0]) > 2 * bar, (name, N, text, score, primed[0][0], bar)
    assert moved >= 4, moved


def test_cached_lm_is_the_definition():
    o = dc.oracle("tied")
    ctx = [7, 9, 7, 11]
    p = dc.CachedLM(o.model, [cc.EOS] + ctx, 3)
    assert p.words.tolist() == [9, 7, 11] and p.keys.shape == (3, 64)          # the last N pairs, oldest first
    h, c = p.zero_state(1)
    pred, _y, h2, _c2, _a, _b = p.predict([cc.EOS], h, c)
    plain = o.model.predict([11], h, c)[0]
    s = dc.THETA * (p.keys @ h2[0])
    w = np.exp(s) / np.exp(s).sum()
    want = (1 - dc.LAM) * plain[0]
    for i, word in enumerate([9, 7, 11]):
        want[word] += dc.LAM * w[i]
    np.testing.assert_allclose(pred[0], want, rtol=1e-12, atol=0)
    assert abs(pred.sum() - 1.0) < 1e-9


# ---------------------------------------------------------------------------------------------- the priming plan
@pytest.mark.parametrize("max_rows", [8, 2])
def test_priming_plan_targets_and_slots(max_rows):
    """the targets of every live step are hist[j + 1]; stored by jlm_prime_cache_frames' rule (slot f - (n_steps - cap), the live prefix)
    a row's entries end at slot cap - 1, hold its last min(len, N) pairs oldest first, and nothing wraps"""
    lengths, N = [7, 0, 40, 1, 7], 16
    rng = np.random.RandomState(3)
    ctxs = [rng.randint(0, 50, size=L).astype(np.int64) for L in lengths]
    hist = [[cc.EOS] + c.tolist() for c in ctxs]
    cap = min(N, max(lengths))
    for ch in jctx.plan_priming(ctxs, max_rows):
        idx = [int(i) for i in ch["idx"]]
        R, S = len(idx), ch["n_steps"]
        assert ch["target"].shape == (S, R) and ch["target"].dtype == np.int32
        k = max(min(cap, S), 1)
        words = np.full((k, R), -1, dtype=np.int64)
        steps = np.full((k, R), -1, dtype=np.int64)
        for f in range(S):
            live = int(ch["n_live"][f])
            for r in range(live):
                j = f - (S - lengths[idx[r]])
                assert ch["word"][f, r] == hist[idx[r]][j] and ch["target"][f, r] == hist[idx[r]][j + 1]
            slot = f - (S - k)
            if slot >= 0:
                words[slot, :live] = ch["target"][f, :live]
                steps[slot, :live] = [f - (S - lengths[idx[r]]) for r in range(live)]
        for r in range(R):
            n = min(lengths[idx[r]], k)
            assert (words[:k - n, r] == -1).all()
            assert words[k - n:, r].tolist() == hist[idx[r]][1:][lengths[idx[r]] - n:]
            assert steps[k - n:, r].tolist() == list(range(lengths[idx[r]] - n, lengths[idx[r]]))


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_before_anything_runs():
    model = types.SimpleNamespace(dev=types.SimpleNamespace(V=10), _primer=lambda: pytest.fail("primed"))
    w2i = {"<unk>": 0, "<eos>": 1}
    for bad in (CacheSpec(8, theta=[0.1, 0.2]), CacheSpec(4097), "cache", 3):
        with pytest.raises(ValueError):
            jctx.check_decode_cache(bad)
        with pytest.raises(ValueError):
            jctx.resolve(model, [[2]], 1, w2i, cache=bad)
    plain = jctx.ContextState(model.dev, None, None, None, None, [1, 4], [0, 0])
    with pytest.raises(ValueError):
        jctx.resolve(model, plain, 2, w2i, cache=CacheSpec(8))               # primed already: prime(cache=) is the way
    assert jctx.resolve(model, [None, []], 2, w2i, cache=CacheSpec(8)) is None   # nothing but empty entries: today's decode
    assert jctx.check_decode_cache(CacheSpec(4096, theta=0.0, lam=0.0)).size == 4096


class _HostCached(jctx.CachedContext):
    """a CachedContext whose host copies are given (no device): what the host-side searches read"""

    def __init__(self, m, n, spec, host, window):
        self.m, self.n, self.spec = m, n, spec
        self.last_host = np.asarray([x[2] for x in host], dtype=np.int32)
        self.has_host = np.ones(n, dtype=np.int32)
        self._host, self._window = host, window

    def numpy(self):
        return np.concatenate([x[0] for x in self._host]), np.concatenate([x[1] for x in self._host])

    def cache_numpy(self):
        return self._window


class _HostPlain(jctx.ContextState):
    """a plain ContextState over the same host copies: what decode(context=) is handed without a cache"""

    def __init__(self, cached):
        self.m, self.n, self.last_host, self.has_host = cached.m, cached.n, cached.last_host, cached.has_host
        self.numpy = cached.numpy


def _host_state(d, o, ctxs, N, lam=dc.LAM):
    host, keys, words, cnt = [], [], [], []
    for c in ctxs:
        hist = [cc.EOS] + list(c)
        h, cl = cc.oracle_state(o.model, hist[:-1])
        host.append((h.astype(np.float32), cl.astype(np.float32), hist[-1]))
        k, w = dc.window(o.model, c, N)
        keys.append(np.concatenate([np.zeros((N - len(w), k.shape[1])), k]))
        words.append(np.concatenate([np.full(N - len(w), -1), w]))
        cnt.append(len(w))
    window = (np.asarray(keys, dtype=np.float32), np.asarray(words, dtype=np.int64), np.asarray(cnt, dtype=np.int32))
    return _HostCached(d.model.dev, len(ctxs), CacheSpec(N, theta=dc.THETA, lam=lam), host, window)


@pytest.fixture()
def decoder(monkeypatch):
    fake_hip.install(monkeypatch)
    dc.set_root("tied")
    from jlm_amd.decoder import Decoder
    d = Decoder(1)
    d.perf_timing = False
    return d


def test_host_search_under_the_cache_equals_the_proxy(decoder):
    """beam_width=None over the numpy ABI double: the unpruned host-side search mixes every frame's probabilities by the float64
    definition over the CachedContext's window"""
    d, o = decoder, dc.oracle("tied")
    sents, ctxs = dc.sentences(), dc.contexts("tied")
    pick = [i for i in range(len(sents)) if cc.ids_of(ctxs[i]) and len(sents[i]) <= 4][:3]
    state = _host_state(d, o, [cc.ids_of(ctxs[i]) for i in pick], 16)
    got = d.decode_batch([sents[i] for i in pick], beam_width=None, context=state)
    primed = d.decode_batch([sents[i] for i in pick], beam_width=None, context=_host_state(d, o, [cc.ids_of(ctxs[i]) for i in pick], 16, lam=0.0))
    # lam = 0 returns what decode(context=) returns for the plain state, ==
    assert primed == d.decode_batch([sents[i] for i in pick], beam_width=None, context=_HostPlain(state))
    for i, g, p in zip(pick, got, primed):
        want = dc.cached_decode(o, sents[i], ctxs[i], 16, beam_width=None)
        assert [w for _, w in g] == [w for _, w in want]
        np.testing.assert_allclose([x for x, _ in g], [x for x, _ in want], rtol=2e-6, atol=2e-5)
        # lam = 0: what decode(context=) returns
        plain = cc.primed_decode(o, sents[i], ctxs[i], beam_width=None)
        np.testing.assert_allclose([x for x, _ in p], [x for x, _ in plain], rtol=2e-6, atol=2e-5)
        assert [x for x, _ in g] != [x for x, _ in p]


def test_decoders_refuse_the_cache(decoder):
    d, o = decoder, dc.oracle("tied")
    state = _host_state(d, o, [[5, 6]], 16)
    spec = CacheSpec(16, theta=dc.THETA, lam=dc.LAM)
    text = dc.sentences()[1]
    for call in (lambda: d.decode(text, vocab_select=True, context=state),
                 lambda: d.decode(text, context=state, cache=spec),
                 lambda: d.decode(text, context=[5, 6], cache=CacheSpec(16, theta=[0.1, 0.2])),
                 lambda: d.decode(text, context=[5, 6], cache=CacheSpec(5000)),
                 lambda: d.decode_predict(text, context=state),
                 lambda: d.decode_predict(text, context=[5, 6], cache=spec),
                 lambda: d.decode_predict_batch([text], context=state)):
        with pytest.raises(ValueError):
            call()
    d.compat_quirks = True
    with pytest.raises(ValueError):
        d.decode(text, context=state)
    d.compat_quirks = False
    from jlm_amd import shard
    with pytest.raises(ValueError):
        shard.decode_sharded(d, [text], 0, 1, context=state)
    with pytest.raises(ValueError):
        shard.decode_sharded(d, [text], 0, 1, context=[[5, 6]], cache=spec)
    from jlm_amd.decoder_dynamic import DynamicDecoder
    dd = DynamicDecoder(1)
    with pytest.raises(ValueError):
        dd.decode(text, vocab_select=True, context=_host_state(dd, o, [[5, 6]], 16))
    from jlm_amd.decoder_char import CharRNNDecoder
    from jlm_amd.decoder_ngram import NGramDecoder
    for cls in (CharRNNDecoder, NGramDecoder):
        with pytest.raises(ValueError):
            cls.decode(object.__new__(cls), text, cache=spec)


# ---------------------------------------------------------------------------------------------- the eval harness
def test_eval_flags_and_log_name():
    from jlm_amd import eval as jeval
    p = jeval.build_parser()
    a = p.parse_args([])
    assert a.cache == 0 and a.theta == 0.3 and a.lam == 0.1
    a = p.parse_args(["-cw", "3", "--cache", "100", "--theta", "0.5", "--lam", "0.2"])
    assert (a.cache, a.theta, a.lam) == (100, 0.5, 0.2)
    ev = object.__new__(jeval.Evaluator)
    ev.args, ev.context_words, ev.cut_last, ev.cache = a, 3, 0, None
    plain = ev.log_name()
    ev.cache = CacheSpec(100, theta=0.5, lam=0.2)
    assert ev.log_name() == plain[:-len(".txt")] + "_cache_100.txt"        # without --cache the name is what it was
