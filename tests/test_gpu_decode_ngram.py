"""GPU: conversion under an n-gram mixture, end to end (Decoder.decode / decode_batch(ngram=); csrc ngram_cell_patch_kernel, the
mixed sequence of jlm_decode_frames) against the UNMODIFIED oracle behind the proxy of tests/decode_ngram_cases.py.

Bars: context_cases.check_nbest's (equal list lengths, identical 1-best words, every score within rtol 2e-6 / atol 2e-5), the atol
widened by decode_ngram_budget.word_bar per word of the path; ``==`` wherever two calls must enqueue the same launches or differ only
in what the kernels may not depend on."""
import pytest

torch = pytest.importorskip("torch")
from jlm_amd.ngram import NGramMix                                       # noqa: E402
from tests import context_cases as cc                                    # noqa: E402
from tests import decode_ngram_cases as nc                               # noqa: E402
from tests.decode_ngram_budget import score_bar                          # noqa: E402
from tests.poison import FILLS, bits, fill_tensor, first_difference      # noqa: E402
from tests.test_gpu_context import decoder                               # noqa: E402

pytestmark = pytest.mark.gpu

SENTS = cc.sentences()
_WANT = {}


def want(name, order, beam, i, with_ctx):
    """the yardstick's n-best of input i (computed once, shared by the tests)"""
    key = (name, order, beam, i, with_ctx)
    if key not in _WANT:
        ctx = nc.contexts(name)[i] if with_ctx else None
        _WANT[key] = nc.mixed_decode(cc.oracle(name), SENTS[i], ctx, nc.mix(name, order), beam_width=beam)
    return _WANT[key]


def check(got, ref, tag):
    assert len(got) == len(ref), tag
    assert got[0][1] == ref[0][1], (tag, got[0], ref[0])
    worst = 0.0
    for (g, gw), (w, _ww) in zip(got, ref):
        bar = score_bar(w, len(gw))
        worst = max(worst, abs(g - w) / bar)
        assert abs(g - w) <= bar, (tag, g, w, bar)
    return worst


@pytest.mark.parametrize("order", nc.ORDERS)
@pytest.mark.parametrize("name", list(cc.MODELS))
def test_against_the_mixed_oracle(name, order):
    d, mix, ctxs = decoder(name), nc.mix(name, order), nc.contexts(name)
    state = d.model.prime([cc.ids_of(c) for c in ctxs])
    assert state.tail_host.tolist() == [([-1, cc.EOS] + cc.ids_of(c))[-2:] for c in ctxs]
    worst = 0.0
    for beam in cc.BEAMS:
        plain = d.decode_batch(SENTS, beam_width=beam, ngram=mix)
        lists = d.decode_batch(SENTS, beam_width=beam, context=ctxs, ngram=mix)
        assert d.decode_batch(SENTS, beam_width=beam, context=state, ngram=mix) == lists      # a primed ContextState: the same launches
        for i in range(len(SENTS)):
            worst = max(worst, check(plain[i], want(name, order, beam, i, False), (name, order, beam, i, "no context")))
            worst = max(worst, check(lists[i], want(name, order, beam, i, True), (name, order, beam, i, "context")))
    print(name, "order", order, "largest share of the bar: %.3f" % worst)
    i = 4
    o = cc.oracle(name)
    check(d.decode(SENTS[i], beam_width=5, ngram=mix), want(name, order, 5, i, False), (name, "decode"))
    check(d.decode(SENTS[i], beam_width=5, context=[o.i2w[w] for w in cc.ids_of(ctxs[i])], ngram=mix), want(name, order, 5, i, True),
          (name, "strings"))


def test_the_mixture_changes_the_result():
    d = decoder("tied")
    plain = d.decode_batch(SENTS, beam_width=5)
    mixed = d.decode_batch(SENTS, beam_width=5, ngram=nc.mix("tied", 3))
    assert sum(a[0][1] != b[0][1] for a, b in zip(plain, mixed)) >= 4


@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_no_ngram_is_todays_decode(name):
    d, ctxs = decoder(name), nc.contexts(name)
    plain, primed = d.decode_batch(SENTS, beam_width=5), d.decode_batch(SENTS, beam_width=5, context=ctxs)
    mixed = d.decode_batch(SENTS, beam_width=5, ngram=nc.mix(name, 3))          # a mixed batch in between leaves nothing behind
    assert mixed != plain
    assert d.decode_batch(SENTS, beam_width=5, ngram=None) == plain
    assert d.decode_batch(SENTS, beam_width=5, context=ctxs, ngram=None) == primed
    assert d.decode(SENTS[4], beam_width=5, ngram=None) == plain[4]


@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_chunks_and_reuse(name, monkeypatch):
    d, mix, ctxs = decoder(name), nc.mix(name, 3), nc.contexts(name)
    whole = d.decode_batch(SENTS, beam_width=5, context=ctxs, ngram=mix)
    assert d.decode_batch(SENTS, beam_width=5, context=ctxs, ngram=mix) == whole
    n_tables = len(mix.table._dev)
    monkeypatch.setattr(d, "max_batch", 4)
    assert len(d._chunks(SENTS, 5)) >= 3
    assert d.decode_batch(SENTS, beam_width=5, context=ctxs, ngram=mix) == whole
    assert len(mix.table._dev) == n_tables == 1                            # the table's device tensors are made once
    # another lambda over the same table: another result, the same tensors
    other = NGramMix(mix.table, 0.1)
    assert other.table is mix.table and d.decode_batch(SENTS, beam_width=5, context=ctxs, ngram=other) != whole


@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_root_histories_are_rewritten_every_batch(name):
    """a decode under the mixture does not depend on what its new buffers held before the call (tests/poison.py's fills)"""
    d, mix, ctxs = decoder(name), nc.mix(name, 3), nc.contexts(name)
    clean = d.decode_batch(SENTS, beam_width=5, context=ctxs, ngram=mix)
    for fill in FILLS:
        filled = 0
        for p in d._engine.plans:
            bufs = getattr(p, "ngram_bufs", None)
            if bufs is not None and not p.busy:
                fill_tensor(bufs.root_hist, fill)
                fill_tensor(bufs.host, fill)
                filled += 1
        assert filled >= 1
        torch.cuda.synchronize()
        got = d.decode_batch(SENTS, beam_width=5, context=ctxs, ngram=mix)
        assert bits(got) == bits(clean), "the n-best depends on a buffer's earlier contents (fill %s): %s" % (
            fill.name, first_difference(got, clean))
