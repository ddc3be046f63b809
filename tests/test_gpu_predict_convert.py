"""GPU: conversion of an unfinished reading end to end (Decoder.decode_predict / decode_predict_batch; csrc/jlm_tail.hip behind
jlm_decode_frames) against the UNMODIFIED oracle listened to by tests/predict_cases.py.

The five models of tests/context_cases.MODELS, its 12 inputs and one empty input, beams 1 / 5 / 17, topN 10, with and without its
contexts.  Bars: conversions ``==`` decode_batch's; predictions of the yardstick's length, sorted scores within the suite's bar (rtol
2e-6 / atol 2e-5), the same words at every position whose yardstick score is more than 1e-4 from both neighbours (the 11th candidate
included; 1e-4 is above the bar for every score below 40) -- at most 2 positions per (model, beam) are closer
(tests/test_predict_convert_cpu.py::test_separation_condition asserts that cap on the CPU)."""
import contextlib
import io
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import config as jconfig, synth            # noqa: E402
from tests import context_cases as cc                   # noqa: E402
from tests import predict_cases as pc                   # noqa: E402

pytestmark = pytest.mark.gpu

TEXTS = pc.inputs()
_DEC = {}


def decoder(name):
    """the model's decoder, loaded once for the module"""
    if name not in _DEC:
        cc.set_root(name)
        from jlm_amd.decoder import Decoder
        _DEC[name] = Decoder(1)
    return _DEC[name]


@pytest.mark.parametrize("with_ctx", [False, True], ids=["plain", "context"])
@pytest.mark.parametrize("name", list(cc.MODELS))
def test_against_the_yardstick(name, with_ctx):
    d = decoder(name)
    ctxs = pc.contexts(cc.MODELS[name][0]) if with_ctx else None
    for beam in cc.BEAMS:
        got = d.decode_predict_batch(TEXTS, topN=pc.TOPN, beam_width=beam, context=ctxs)
        assert [c for c, _p in got] == d.decode_batch(TEXTS, topN=pc.TOPN, beam_width=beam, context=ctxs), (name, beam)
        exempt = 0
        for i, ((conv, pred), (yconv, cands)) in enumerate(zip(got, pc.yardstick(name, beam, with_ctx))):
            if len(TEXTS[i]):
                cc.check_nbest(conv, yconv, (name, beam, i))
            else:
                assert conv == [(0.0, [])]
            exempt += pc.check_predictions(pred, cands, (name, beam, with_ctx, i))
        assert exempt <= pc.MAX_EXEMPT, (name, beam, exempt)


@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_permuted_chunked_and_single(name):
    d = decoder(name)
    ctxs = pc.contexts(cc.MODELS[name][0])
    ref = d.decode_predict_batch(TEXTS, topN=pc.TOPN, beam_width=5, context=ctxs)
    perm = list(np.random.RandomState(3).permutation(len(TEXTS)))
    got = d.decode_predict_batch([TEXTS[i] for i in perm], topN=pc.TOPN, beam_width=5, context=[ctxs[i] for i in perm])
    assert got == [ref[i] for i in perm]
    keep = d.max_batch
    d.max_batch = 5                                                                   # 12 inputs in 3 chunks, then the empty one
    try:
        assert d.decode_predict_batch(TEXTS, topN=pc.TOPN, beam_width=5, context=ctxs) == ref
    finally:
        d.max_batch = keep
    for i in (0, 4, 12):
        one = d.decode_predict(TEXTS[i], topN=pc.TOPN, beam_width=5, context=ctxs[i])
        assert one == ref[i] and one[0] == d.decode(TEXTS[i], topN=pc.TOPN, beam_width=5, context=ctxs[i])
    # the result does not depend on the chunk of the selection
    d._engine.PREDICT_CHUNK = 64
    try:
        assert d.decode_predict_batch(TEXTS, topN=pc.TOPN, beam_width=5, context=ctxs) == ref
    finally:
        d._engine.PREDICT_CHUNK = 0
    assert d.decode_predict_batch(TEXTS, topN=3, beam_width=5, context=ctxs) == [(c[:3], p[:3]) for c, p in ref]


@pytest.mark.parametrize("name", ["tied", "dsoftmax"])
def test_one_kana_input_against_predict_reading(name):
    """a one-kana input has the tail start 0 alone: a prediction is one word after the history, and its score is predict_reading's
    -log p of that word (the same distribution through the row kernels of jlm_topk.hip), within the suite's bar"""
    d = decoder(name)
    ctxs = pc.contexts(cc.MODELS[name][0])
    kana = sorted({t[0] for t in TEXTS if t})
    n = 0
    for ch in kana:
        for ctx in (None, ctxs[5], ctxs[2]):
            _conv, pred = d.decode_predict(ch, topN=pc.TOPN, beam_width=5, context=ctx)
            ids, logp = d.model.predict_reading([[cc.EOS] + cc.ids_of(ctx)], [ch], n=64)[0]
            table = {int(w): -float(lp) for w, lp in zip(ids, logp)}
            for score, words in pred:
                assert len(words) == 1
                w = d.w2i[words[0]]
                if w in table:
                    np.testing.assert_allclose(score, table[w], rtol=2e-6, atol=2e-5)
                    n += 1
    assert n >= 20


def test_eval_cut_last(fx, monkeypatch, tmp_path):
    from jlm_amd import eval as jeval
    from tests import golden_cases as gc
    f = fx("small-tied")
    synth.write_test_corpus(f["root"], f["lexicon"], f["cfg"]["vocab_size"], **gc.EVAL_CORPUS)
    jconfig.set_root(f["root"])
    monkeypatch.chdir(tmp_path)
    os.makedirs("eval", exist_ok=True)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        best, nbest, miss = jeval.main(["-e", "1", "-es", "12", "-b", "10", "--batch", "16", "--cut_last", "1"])
    assert best + nbest + miss == 12 and "pred_best_hit %d pred_nbest_hit %d pred_miss %d eval_size 12" % (best, nbest, miss) in buf.getvalue()
    assert any(n.endswith("_cut_1.txt") for n in os.listdir("eval"))
    with contextlib.redirect_stdout(io.StringIO()):
        again = jeval.main(["-e", "1", "-es", "12", "-b", "10", "--batch", "1", "--cut_last", "1", "-cw", "1"])
    assert sum(again) == 12
