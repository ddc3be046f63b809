"""GPU: conversion under the continuous cache, end to end (Decoder.decode / decode_batch(context=, cache=), LSTM_Model.prime(cache=);
csrc jlm_prime_cache_frames, cache_cell_query_kernel, cache_cell_patch_kernel, the cached sequence of jlm_decode_frames) against the
UNMODIFIED oracle behind the proxy of tests/decode_cache_cases.py.

Bars: context_cases.check_nbest's (equal list lengths, identical 1-best words, every score within rtol 2e-6 / atol 2e-5), the atol
widened by decode_cache_budget.word_bar per word of the path; ``==`` wherever two calls must enqueue the same launches or differ only
in what the kernels may not depend on."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd.cache import CacheSpec                                      # noqa: E402
from jlm_amd.context import CachedContext                                # noqa: E402
from tests import context_cases as cc                                    # noqa: E402
from tests import decode_cache_cases as dc                               # noqa: E402
from tests.decode_cache_budget import word_bar                           # noqa: E402
from tests.test_gpu_context import decoder                               # noqa: E402

pytestmark = pytest.mark.gpu

SENTS = cc.sentences()


def spec(N, lam=dc.LAM):
    return CacheSpec(N, theta=dc.THETA, lam=lam)


def check(d, got, want, N, tag):
    m = d.model.dev
    assert len(got) == len(want), tag
    assert got[0][1] == want[0][1], (tag, got[0], want[0])
    wb = word_bar(bool(m.split_lstm), m.H, N, dc.THETA)
    worst = 0.0
    for (g, gw), (w, _ww) in zip(got, want):
        bar = 2e-5 + 2e-6 * abs(w) + wb * max(len(gw), 1)
        worst = max(worst, abs(g - w) / bar)
        assert abs(g - w) <= bar, (tag, g, w, bar)
    return worst


@pytest.mark.parametrize("name", list(cc.MODELS))
def test_against_the_cached_oracle(name):
    d, o, ctxs = decoder(name), cc.oracle(name), dc.contexts(name)
    worst = 0.0
    for N in dc.SIZES:
        state = d.model.prime([cc.ids_of(c) for c in ctxs], cache=spec(N))
        assert isinstance(state, CachedContext) and state.cap == min(N, 40)
        assert state.count_host.tolist() == [min(len(cc.ids_of(c)), N) for c in ctxs]
        for beam in cc.BEAMS:
            got = d.decode_batch(SENTS, beam_width=beam, context=state)
            if beam == 5:
                assert got == d.decode_batch(SENTS, beam_width=beam, context=ctxs, cache=spec(N))       # word lists primed by the decoder
            for s, c, g in zip(SENTS, ctxs, got):
                worst = max(worst, check(d, g, dc.cached_decode(o, s, c, N, beam_width=beam), N, (name, N, beam, s, c)))
    print(name, "largest share of the bar: %.3f" % worst)
    i = 4
    want = dc.cached_decode(o, SENTS[i], ctxs[i], 64, beam_width=5)
    check(d, d.decode(SENTS[i], beam_width=5, context=ctxs[i], cache=spec(64)), want, 64, (name, "decode"))
    check(d, d.decode(SENTS[i], beam_width=5, context=[o.i2w[w] for w in cc.ids_of(ctxs[i])], cache=spec(64)), want, 64, (name, "strings"))


def test_the_cache_changes_the_result():
    d, ctxs = decoder("tied"), dc.contexts("tied")
    primed = d.decode_batch(SENTS, beam_width=5, context=ctxs)
    cached = d.decode_batch(SENTS, beam_width=5, context=ctxs, cache=spec(16))
    assert sum(a[0][1] != b[0][1] for a, b in zip(primed, cached)) >= 4
    # sentences whose window is empty, inside a cached batch: the decode without a cache
    for i, c in enumerate(ctxs):
        if not cc.ids_of(c):
            assert cached[i] == primed[i], i


@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_lam_zero_and_no_cache_are_todays_decode(name):
    d, ctxs = decoder(name), dc.contexts(name)
    plain = d.decode_batch(SENTS, beam_width=5, context=ctxs)
    assert d.decode_batch(SENTS, beam_width=5, context=ctxs, cache=None) == plain
    assert d.decode_batch(SENTS, beam_width=5, context=ctxs, cache=spec(16, lam=0.0)) == plain
    assert d.decode_batch(SENTS, beam_width=5, context=d.model.prime([cc.ids_of(c) for c in ctxs], cache=spec(16, lam=0.0))) == plain
    # every window empty: nothing to prime, the decode without a context
    empty = d.model.prime([[] for _ in SENTS], cache=spec(16))
    assert d.decode_batch(SENTS, beam_width=5, context=empty) == d.decode_batch(SENTS, beam_width=5)


@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_reusing_a_cached_context(name, monkeypatch):
    d, ctxs = decoder(name), dc.contexts(name)
    state = d.model.prime([cc.ids_of(c) for c in ctxs], cache=spec(16))
    whole = d.decode_batch(SENTS, beam_width=5, context=state)
    assert d.decode_batch(SENTS, beam_width=5, context=state) == whole
    perm = np.random.RandomState(9).permutation(len(SENTS)).tolist()
    shuffled = [SENTS[i] for i in perm]                      # (row i of the state goes with input i of the call, whatever the input is)
    assert d.decode_batch(shuffled, beam_width=5, context=state) == d.decode_batch(shuffled, beam_width=5, context=ctxs, cache=spec(16))
    monkeypatch.setattr(d, "max_batch", 4)
    assert len(d._chunks(SENTS, 5)) >= 3
    assert d.decode_batch(SENTS, beam_width=5, context=state) == whole


@pytest.mark.parametrize("name", ["tied", "tied-h512"])
def test_priming_with_a_cache_keeps_the_primed_state(name):
    d, ctxs = decoder(name), dc.contexts(name)
    ids = [cc.ids_of(c) for c in ctxs]
    plain, cached = d.model.prime(ids), d.model.prime(ids, cache=spec(16))
    for a in ("h", "c", "last", "has"):
        assert torch.equal(getattr(plain, a), getattr(cached, a)), a
    # the window against the oracle's own states: the predict API's bars (tests/test_gpu_context.py)
    o = cc.oracle(name)
    hh, ww, cnt = cached.cache_numpy()
    for r, c in enumerate(ids):
        keys, words = dc.window(o.model, c, 16)
        assert cnt[r] == len(words) and ww[r, 16 - cnt[r]:].tolist() == words.tolist(), r
        np.testing.assert_allclose(hh[r, 16 - cnt[r]:], keys, rtol=1e-4, atol=1e-5, err_msg=str(r))


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_the_window_is_what_cached_scoring_leaves(precision, monkeypatch):
    """an equal-length batch: prime(cache=)'s hist / words are torch.equal to the CacheState score_streams_cached leaves after the same
    steps -- the state set each step wrote, copied bit for bit, in both state-row formats (split rows and f32)"""
    monkeypatch.setenv("JLM_PRECISION", precision)
    cc.set_root("tied")
    from jlm_amd.decoder import Decoder
    m = Decoder(1).model
    assert bool(m.dev.split_lstm) == (precision == "f16x3")
    rng = np.random.RandomState(4)
    n, R = 9, 7
    ctxs = rng.randint(2, m.dev.V, size=(R, n))
    for N in (n, 4):                                                       # the whole context, and a window that truncates it
        state = m.prime(ctxs.tolist(), cache=spec(N))
        inputs = np.concatenate([np.full((R, 1), cc.EOS), ctxs[:, :-1]], axis=1)
        left = m.score_streams_cached(inputs, ctxs, CacheSpec(N, theta=dc.THETA, lam=dc.LAM)).state
        assert state.cap == N == left.count and state.count_host.tolist() == [N] * R
        assert torch.equal(state.hist.view(torch.int32), left.hist.view(torch.int32))
        assert torch.equal(state.words, left.words)
