"""GPU: conversion under a memory, end to end (Decoder.decode / decode_batch(memory=); csrc memory_gather_rows_kernel, jlm_memory_topk,
memory_cell_patch_kernel, the memory's sequence of jlm_decode_frames) against the UNMODIFIED oracle behind the proxy of
tests/decode_memory_cases.py.  The device's memory holds the yardstick's own float64 keys, rounded once to the model's state-row format
(tests/test_gpu_cache_rows.py encode): what is under test is the decode under a memory, not Memory.build, and a
memory built on the device is not entry for entry the oracle's on every model -- the H = 512 model's random recurrence amplifies the
state rows' rounding along the 813-step stream (entry 0 differs from the oracle's by 8e-8, entry 10 by 6.5e-7, the largest by more than
a unit), which no bar on a score can follow.  On the H = 64 models the two memories agree, and one test decodes under the built one.

K = 1 024 >= N (every entry votes: no neighbour set to disagree about): context_cases.check_nbest's bars -- equal list lengths,
identical 1-best words, every score within rtol 2e-6 / atol 2e-5 -- the atol widened by decode_memory_budget.word_bar per word.
K = 16: the smallest float64 gap between the 16th and the 17th score is at or below the score bars, so an oracle cannot be expected to
pick the device's neighbour set on every row.  Every returned path's score must lie inside the float64 interval of that path's chain
score (decode_memory_cases.chain_interval: entries within twice the score bar of the boundary in or out, whichever raises or lowers the
word's mass), widened by the same bars; on the separable inputs the n-best strings must be the oracle's.
``==`` wherever two calls must enqueue the same launches or differ only in what the kernels may not depend on."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import memory as M                                          # noqa: E402
from jlm_amd.engine import _MemoryBufs                                   # noqa: E402
from tests import context_cases as cc                                    # noqa: E402
from tests import decode_memory_cases as mc                              # noqa: E402
from tests.decode_memory_budget import RTOL, path_atol                   # noqa: E402
from tests.poison import FILLS, bits, fill_tensor, first_difference      # noqa: E402
from tests.test_gpu_cache_rows import H_SCALE, encode                    # noqa: E402
from tests.test_gpu_context import decoder                               # noqa: E402

pytestmark = pytest.mark.gpu

SENTS = cc.sentences()
_MEM, _WANT = {}, {}


def memory(name):
    """the device's memory of model ``name``: the yardstick's keys in the model's state-row format (made once for the module)"""
    if name not in _MEM:
        dm = decoder(name).model.dev
        _ids, keys, words = mc.store(name)
        assert not dm.split_lstm or float(dm.h_scale) == H_SCALE
        raw, _val = encode(keys, bool(dm.split_lstm))
        with dm._ctx():
            _MEM[name] = M.Memory(dm, torch.from_numpy(raw).to(dm.device), torch.from_numpy(words.astype(np.int32)).to(dm.device))
    return _MEM[name]


def mix(name, K, lam=mc.LAM):
    return M.MemoryMix(memory(name), theta=mc.THETA, lam=lam, k=K)


def want(name, K, beam, i, with_ctx):
    """the yardstick's (n-best, separable) of input i (computed once, shared by the tests)"""
    key = (name, K, beam, i, with_ctx)
    if key not in _WANT:
        ctx = mc.contexts(name)[i] if with_ctx else None
        _WANT[key] = mc.memory_decode(cc.oracle(name), SENTS[i], ctx, name, K, beam_width=beam)
    return _WANT[key]


def bar_of(d, n_q, score, n_words):
    dm = d.model.dev
    return path_atol(bool(dm.split_lstm), int(dm.H), n_q, mc.THETA, n_words) + RTOL * abs(score)


def check(d, got, ref, n_q, tag):
    assert len(got) == len(ref), tag
    assert got[0][1] == ref[0][1], (tag, got[0], ref[0])
    worst = 0.0
    for (g, gw), (w, _ww) in zip(got, ref):
        bar = bar_of(d, n_q, w, len(gw))
        worst = max(worst, abs(g - w) / bar)
        assert abs(g - w) <= bar, (tag, g, w, bar)
    return worst


@pytest.mark.parametrize("name", list(cc.MODELS))
def test_against_the_memory_oracle(name):
    d, mx, ctxs = decoder(name), mix(name, mc.K_ALL), mc.contexts(name)
    n_q = mx.n_q
    assert n_q == memory(name).N < mc.K_ALL
    worst = 0.0
    for beam in cc.BEAMS:
        plain = d.decode_batch(SENTS, beam_width=beam, memory=mx)
        lists = d.decode_batch(SENTS, beam_width=beam, context=ctxs, memory=mx)
        for i in range(len(SENTS)):
            worst = max(worst, check(d, plain[i], want(name, mc.K_ALL, beam, i, False)[0], n_q, (name, beam, i, "no context")))
            worst = max(worst, check(d, lists[i], want(name, mc.K_ALL, beam, i, True)[0], n_q, (name, beam, i, "context")))
    print(name, "K >= N: largest share of the bar %.3f" % worst)
    i = 4
    check(d, d.decode(SENTS[i], beam_width=5, memory=mx), want(name, mc.K_ALL, 5, i, False)[0], n_q, (name, "decode"))
    check(d, d.decode(SENTS[i], beam_width=5, context=cc.ids_of(ctxs[i]), memory=mx), want(name, mc.K_ALL, 5, i, True)[0], n_q, (name, "ctx"))


@pytest.mark.parametrize("name", list(cc.MODELS))
def test_k16_scores_lie_in_their_chain_intervals_and_separable_inputs_agree(name):
    d, o, mx, ctxs = decoder(name), cc.oracle(name), mix(name, mc.K_SMALL), mc.contexts(name)
    _ids, keys, words = mc.store(name)
    separable = open_intervals = paths = 0
    for with_ctx in (False, True):
        got = d.decode_batch(SENTS, beam_width=5, **(dict(context=ctxs) if with_ctx else {}), memory=mx)
        for i, nbest in enumerate(got):
            hist = [cc.EOS] + (cc.ids_of(ctxs[i]) if with_ctx else [])
            for score, path in nbest:
                lo, _mid, hi = mc.chain_interval(o.model, hist, cc.path_ids(o, path), keys, words, mc.K_SMALL)
                paths += 1
                open_intervals += hi > lo
                assert lo - bar_of(d, mc.K_SMALL, lo, len(path)) <= score <= hi + bar_of(d, mc.K_SMALL, hi, len(path)), \
                    (name, with_ctx, i, path, score, lo, hi)
            ref, sep = want(name, mc.K_SMALL, 5, i, with_ctx)
            if sep:
                separable += 1
                assert [w for _s, w in nbest] == [w for _s, w in ref], (name, with_ctx, i)
                check(d, nbest, ref, mc.K_SMALL, (name, with_ctx, i, "separable"))
    assert separable >= 3
    print(name, "K = 16: %d paths, %d with an open interval, %d separable inputs of %d" % (paths, open_intervals, separable, 2 * len(SENTS)))


@pytest.mark.parametrize("name", ["tied", "vtable"])
def test_a_memory_built_on_the_device(name):
    """Memory.build over the stream the yardstick's store was made from: the same entries to the accuracy of a state row on these
    models, and the decode under it holds against the same oracle"""
    d = decoder(name)
    x, y = mc.streams(name)
    built = M.Memory.build(d.model, x, y, 50)
    _ids, keys, words = mc.store(name)
    dk, dw = built.numpy()
    assert built.N == len(words) and np.array_equal(dw, words) and np.abs(dk - keys).max() <= 2e-6
    mx = M.MemoryMix(built, theta=mc.THETA, lam=mc.LAM, k=mc.K_ALL)
    got = d.decode_batch(SENTS, beam_width=5, memory=mx)
    for i in range(len(SENTS)):
        check(d, got[i], want(name, mc.K_ALL, 5, i, False)[0], mx.n_q, (name, i, "built"))


def test_the_memory_changes_the_result():
    d = decoder("tied")
    plain = d.decode_batch(SENTS, beam_width=5)
    for K in (mc.K_SMALL, mc.K_ALL):
        mixed = d.decode_batch(SENTS, beam_width=5, memory=mix("tied", K))
        assert sum(a[0][1] != b[0][1] for a, b in zip(plain, mixed)) >= 4


@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_no_memory_is_todays_decode(name):
    d, ctxs = decoder(name), mc.contexts(name)
    plain, primed = d.decode_batch(SENTS, beam_width=5), d.decode_batch(SENTS, beam_width=5, context=ctxs)
    mixed = d.decode_batch(SENTS, beam_width=5, memory=mix(name, mc.K_SMALL))       # a batch under a memory in between leaves nothing behind
    assert mixed != plain
    zero = mix(name, mc.K_SMALL, lam=0.0)
    for kw in (dict(memory=None), dict(memory=zero)):
        assert d.decode_batch(SENTS, beam_width=5, **kw) == plain
        assert d.decode_batch(SENTS, beam_width=5, context=ctxs, **kw) == primed
        assert d.decode(SENTS[4], beam_width=5, **kw) == plain[4]


@pytest.mark.parametrize("K", [mc.K_SMALL, mc.K_ALL])
@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_chunks_permutations_padding_and_the_workspace(name, K, monkeypatch):
    """the same bits with the retrieval's workspace cut to chunks of 32 keys, with the batch permuted, padded with other sentences and cut
    into several device batches"""
    d, mx, ctxs = decoder(name), mix(name, K), mc.contexts(name)
    whole = d.decode_batch(SENTS, beam_width=5, context=ctxs, memory=mx)
    assert d.decode_batch(SENTS, beam_width=5, context=ctxs, memory=mx) == whole
    monkeypatch.setattr(_MemoryBufs, "CHUNK_KEYS", 32)
    assert d.decode_batch(SENTS, beam_width=5, context=ctxs, memory=mx) == whole
    cut = [p for p in d._engine.plans if p.memory_bufs is not None and p.memory_bufs.key == (mx.memory.N, K, 32)]
    assert cut and all(p.memory_bufs.workspace.numel() == p.rmax * (32 + 2 * K) for p in cut)      # the least jlm_memory_topk takes
    monkeypatch.setattr(_MemoryBufs, "CHUNK_KEYS", None)
    perm = np.random.RandomState(3).permutation(len(SENTS))
    got = d.decode_batch([SENTS[i] for i in perm], beam_width=5, context=[ctxs[i] for i in perm], memory=mx)
    assert [got[list(perm).index(i)] for i in range(len(SENTS))] == whole
    pad = cc.synth.make_ragged_sentences(7, 1, 12, seed=5, alphabet=cc.ALPHABET)
    got = d.decode_batch(pad[:3] + SENTS + pad[3:], beam_width=5, context=[None] * 3 + list(ctxs) + [None] * 4, memory=mx)
    assert got[3:3 + len(SENTS)] == whole
    monkeypatch.setattr(d, "max_batch", 4)
    assert len(d._chunks(SENTS, 5)) >= 3
    assert d.decode_batch(SENTS, beam_width=5, context=ctxs, memory=mx) == whole


@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_the_new_buffers_are_rewritten_every_batch(name):
    """a decode under a memory does not depend on what its new buffers held before the call (tests/poison.py's fills)"""
    d, mx, ctxs = decoder(name), mix(name, mc.K_SMALL), mc.contexts(name)
    clean = d.decode_batch(SENTS, beam_width=5, context=ctxs, memory=mx)
    for fill in FILLS:
        filled = 0
        for p in d._engine.plans:
            bufs = getattr(p, "memory_bufs", None)
            if bufs is not None and not p.busy:
                for t in (bufs.q_rows, bufs.s, bufs.ret_words, bufs.workspace, bufs.flags, bufs.h_flags):
                    fill_tensor(t, fill)
                filled += 1
        assert filled >= 1
        torch.cuda.synchronize()
        got = d.decode_batch(SENTS, beam_width=5, context=ctxs, memory=mx)
        assert bits(got) == bits(clean), "the n-best depends on a buffer's earlier contents (fill %s): %s" % (
            fill.name, first_difference(got, clean))


def test_host_side_searches_agree_with_the_oracle(monkeypatch):
    """beam_width=None (the unpruned search) and a sentence whose cells the device beam step cannot hold (_CellTooLarge: the host-side
    search with the beam) mix every frame's probabilities by the float64 definition over Memory.numpy()"""
    name = "tied"
    d, o, mx = decoder(name), cc.oracle(name), mix(name, mc.K_ALL)
    pick = [i for i in range(len(SENTS)) if len(SENTS[i]) <= 4][:3]
    got = d.decode_batch([SENTS[i] for i in pick], beam_width=None, memory=mx)
    for i, g in zip(pick, got):
        ref, _sep = mc.memory_decode(o, SENTS[i], None, name, mc.K_ALL, beam_width=None)
        assert [w for _, w in g] == [w for _, w in ref]
        for (a, aw), (b, _bw) in zip(g, ref):
            assert abs(a - b) <= bar_of(d, mx.n_q, b, len(aw)), (i, a, b)
    device = d.decode_batch(SENTS, beam_width=5, memory=mx)
    monkeypatch.setattr(d, "CAND_LIMIT", 5 * 3)
    heavy = d.decode_batch(SENTS, beam_width=5, memory=mx)
    assert any(h != v for h, v in zip(heavy, device))                      # (some sentence took the host path)
    for i in range(len(SENTS)):
        check(d, heavy[i], want(name, mc.K_ALL, 5, i, False)[0], mx.n_q, (i, "heavy"))


def test_refusals_on_the_device():
    d, other = decoder("tied"), decoder("vtable")
    mx = mix("tied", mc.K_SMALL)
    with pytest.raises(ValueError, match="of this model"):
        other.decode(SENTS[1], memory=mx)
    from jlm_amd.cache import CacheSpec
    with pytest.raises(ValueError):
        d.decode(SENTS[1], context=[5, 6], cache=CacheSpec(16, theta=0.5, lam=0.5), memory=mx)
    from tests import decode_ngram_cases as nc
    with pytest.raises(ValueError):
        d.decode(SENTS[1], ngram=nc.mix("tied", 2), memory=mx)
    with pytest.raises(ValueError):
        d.decode_predict(SENTS[1], memory=mx)
