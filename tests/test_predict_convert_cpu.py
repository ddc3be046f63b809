"""CPU: conversion of an unfinished reading (Decoder.decode_predict) -- the reading ranges against a brute-force
scan, the yardstick (tests/predict_cases.py) against the chain rule, the separation of its scores, the host path end to end over the
numpy double of the new op (tests/fake_tail.py), and every refusal."""
import numpy as np
import pytest

from jlm_amd import readings
from tests import context_cases as cc
from tests import fake_tail
from tests import predict_cases as pc


@pytest.fixture()
def fake(monkeypatch):
    return fake_tail.install(monkeypatch)


# ---------------------------------------------------------------------------------------------- reading ranges
def _brute(index, prefix):
    p = readings.to_katakana(prefix)
    eq = [int(i) for r, i in zip(index.readings, index.ids) if r == p]
    ext = [int(i) for r, i in zip(index.readings, index.ids) if r.startswith(p) and len(r) > len(p)]
    return eq, ext


def test_ranges_against_a_brute_force_scan():
    index = pc.index_of("tied")
    rs = sorted(set(index.readings))
    only_exact = [r for r in rs if not any(q.startswith(r) and q != r for q in rs)]
    assert only_exact
    hira = "".join(chr(ord(c) - 0x60) for c in rs[0][:1])
    prefixes = ["", hira, rs[0][:1], rs[3], rs[-1], only_exact[0], rs[0] + "ヷヷ", "zzz"] + rs[5:40:7] + [r[:2] for r in rs[::23]]
    seen = set()
    for p in prefixes:
        lo, mid, hi = index.ranges(p)
        eq, ext = _brute(index, p)
        assert lo <= mid <= hi
        assert index.ids[lo:mid].tolist() == eq and index.ids[mid:hi].tolist() == ext, p
        assert sorted(eq + ext) == index.lookup(p).tolist() and sorted(eq) == index.lookup(p, exact=True).tolist()
        seen.add((bool(eq), bool(ext)))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    assert index.ranges("") == (0, 0, len(index))                       # every word that has a reading extends the empty prefix
    assert index.ranges(hira) == index.ranges(rs[0][:1])                # hiragana folds to katakana
    lo, mid, hi = index.ranges(only_exact[0])
    assert lo < mid == hi


# ---------------------------------------------------------------------------------------------- the yardstick checks itself
@pytest.mark.parametrize("name", ["tied", "dsoftmax"])
def test_yardstick_scores_are_the_chain_rule(name):
    """every yardstick prediction's score = the chain-rule sum of -log p over its words after the history, to 1e-9"""
    o = cc.oracle(name)
    V = cc.MODELS[name][0]
    n = 0
    for with_ctx in (False, True):
        ctxs = pc.contexts(V) if with_ctx else [None] * 13
        for (conv, cands), text, ctx in zip(pc.yardstick(name, 5, with_ctx), pc.inputs(), ctxs):
            assert cands, text
            for score, words in cands[:pc.TOPN]:
                want = cc.chain_nll(o.model, [cc.EOS] + cc.ids_of(ctx), cc.path_ids(o, words)).sum()
                assert abs(score - want) <= 1e-9, (name, text, ctx, words, score, want)
                n += 1
            if len(text):
                assert conv == cc.primed_decode(o, text, ctx, beam_width=5)
    assert n >= 200


def test_yardstick_candidates_are_tail_extensions():
    """a prediction's last word properly extends the tail its path leaves, its other words cover the input in front of it"""
    o, index = cc.oracle("tied"), pc.index_of("tied")
    starts = set()
    for (_conv, cands), text in zip(pc.yardstick("tied", 17, False), pc.inputs()):
        for _score, words in cands[:pc.TOPN]:
            covered = sum(len(readings.reading_of(w) or w) for w in words[:-1])
            tail = readings.to_katakana(text[covered:])
            r = readings.reading_of(words[-1])
            assert covered < len(text) or not text
            assert r.startswith(tail) and len(r) > len(tail), (text, words)
            starts.add(covered)
    assert len(starts) >= 3


@pytest.mark.parametrize("with_ctx", [False, True], ids=["plain", "context"])
@pytest.mark.parametrize("name", list(cc.MODELS))
def test_separation_condition(name, with_ctx):
    """what lets the GPU test compare words: per (model, beam) at most MAX_EXEMPT of the top-10 positions over the 13 inputs have a
    neighbour (the 11th candidate included) within 1e-4"""
    for beam in cc.BEAMS:
        close = sum(pc.separated(cands).count(False) for _conv, cands in pc.yardstick(name, beam, with_ctx))
        assert close <= pc.MAX_EXEMPT, (name, beam, with_ctx, close)


# ---------------------------------------------------------------------------------------------- the host path over the double
def _decoder(name):
    cc.set_root(name)
    from jlm_amd.decoder import Decoder
    d = Decoder(1)
    d.perf_timing = False
    return d


@pytest.mark.parametrize("name", ["tied", "vtable"])
def test_host_path_end_to_end(name, fake):
    dec = _decoder(name)
    texts = pc.inputs()
    for beam in (1, 5):
        got = dec.decode_predict_batch(texts, topN=pc.TOPN, beam_width=beam)
        conv = dec.decode_batch(texts, topN=pc.TOPN, beam_width=beam)
        assert len(got) == len(texts)
        exempt = 0
        for i, ((c, p), (_yc, cands)) in enumerate(zip(got, pc.yardstick(name, beam, False))):
            assert c == conv[i], (name, beam, i)
            exempt += pc.check_predictions(p, cands, (name, beam, i))
        assert exempt <= pc.MAX_EXEMPT
        assert got[-1][0] == [(0.0, [])] and len(got[-1][1]) == pc.TOPN
    # one input, the batch in three chunks, another order: the same lists
    one = dec.decode_predict(texts[4], topN=3, beam_width=5)
    assert one[0] == dec.decode(texts[4], topN=3, beam_width=5) and one[1] == got[4][1][:3]
    dec.max_batch = 5
    assert dec.decode_predict_batch(texts, topN=pc.TOPN, beam_width=5) == got
    dec.max_batch = 1024
    perm = list(reversed(range(len(texts))))
    assert dec.decode_predict_batch([texts[i] for i in perm], topN=pc.TOPN, beam_width=5) == [got[i] for i in perm]
    assert dec.decode_predict_batch([], beam_width=5) == []
    assert dec.decode_predict("", topN=2, beam_width=5) == ([(0.0, [])], got[-1][1][:2])


def test_plans_of_plain_decodes_are_untouched(fake):
    """a predicting batch takes a plan of its own (one more key element, as a left context does)"""
    dec = _decoder("tied")
    texts = pc.inputs()[:4]
    dec.decode_batch(texts, beam_width=5)
    keys = {p.key for p in dec._engine.plans}
    dec.decode_predict_batch(texts, topN=7, beam_width=5)
    new = {p.key for p in dec._engine.plans} - keys
    assert len(new) == 1 and all(len(k) == 7 for k in keys)
    (k,) = new
    assert len(k) == 9 and k[7] is False and k[8] == 7 and k[:7] in keys


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch(fake, monkeypatch):
    dec = _decoder("tied")
    texts = pc.inputs()[:3]
    launched = []
    monkeypatch.setattr(dec._engine, "submit", lambda *a, **k: launched.append(1))
    monkeypatch.setattr(dec.model, "prime", lambda *a, **k: launched.append(2))
    with pytest.raises(ValueError):
        dec.decode_predict_batch(texts, beam_width=None)
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError):
            dec.decode_predict_batch(texts, topN=bad)
    with pytest.raises(ValueError):
        dec.decode_predict_batch(texts, beam_width=0)
    dec.compat_quirks, dec.lattice_vocab = True, [1, 2, 3]
    with pytest.raises(ValueError):
        dec.decode_predict(texts[0])
    dec.compat_quirks, dec.lattice_vocab = False, None
    dec.CAND_LIMIT = 1                                       # every cell is too large for the device beam step
    with pytest.raises(ValueError) as e:
        dec.decode_predict_batch(texts, beam_width=5, context=[[5], [6], [7]])
    assert repr(texts[0]) in str(e.value) and "0 (" in str(e.value)
    dec.CAND_LIMIT = None
    with pytest.raises(TypeError):
        dec.decode_predict_batch(texts, vocab_select=True)   # there is no such argument
    assert not launched


def test_other_decoders_raise_type_error(fake):
    cc.set_root("tied")
    from jlm_amd.decoder_dynamic import DynamicDecoder
    from jlm_amd.decoder_char import CharRNNDecoder
    from jlm_amd.decoder_ngram import NGramDecoder
    d = DynamicDecoder(1)
    with pytest.raises(TypeError):
        d.decode_predict("アイ")
    with pytest.raises(TypeError):
        d.decode_predict_batch(["アイ"])
    for cls in (CharRNNDecoder, NGramDecoder):
        obj = cls.__new__(cls)                               # (the refusal needs no model)
        with pytest.raises(TypeError):
            obj.decode_predict("アイ")
        with pytest.raises(TypeError):
            obj.decode_predict_batch(["アイ"])


def test_engine_refuses_malformed_spans(fake):
    dec = _decoder("tied")
    from jlm_amd.lattice import BatchLattice
    texts = pc.inputs()[:2]
    lat = BatchLattice(dec._builder, texts, 3)
    z = np.zeros(0, dtype=np.int32)
    ids = np.zeros(4, dtype=np.int32)
    for sp, n in (((np.array([0, 0]), z, z, z), 3),                                  # sp_off of the wrong length
                  ((np.array([0, 0, 0]), z, z, z), 0), ((np.array([0, 0, 0]), z, z, z), 65),
                  ((np.array([0, 1, 1]), np.array([len(texts[0])]), np.array([0]), np.array([2])), 3),   # a frame past the sentence
                  ((np.array([0, 1, 1]), np.array([0]), np.array([3]), np.array([2])), 3)):              # lo > hi
        with pytest.raises(ValueError):
            dec._engine.submit(lat, "static", predict=(sp, ids, dec.i2w, n))
    with pytest.raises(ValueError):
        dec._engine.submit(lat, "static", vocab=(np.array([1]), np.array([0, 1, 1])), predict=((np.array([0, 0, 0]), z, z, z), ids, dec.i2w, 3))
    assert not any(p.busy for p in dec._engine.plans)


# ---------------------------------------------------------------------------------------------- eval harness and command line
def test_eval_cut_last_counts_add_up(fx, fake, monkeypatch, tmp_path, capsys):
    import os
    from jlm_amd import config as jconfig, eval as jeval, synth
    from tests import golden_cases as gc
    f = fx("small-tied")
    synth.write_test_corpus(f["root"], f["lexicon"], f["cfg"]["vocab_size"], **gc.EVAL_CORPUS)
    jconfig.set_root(f["root"])
    monkeypatch.chdir(tmp_path)
    os.makedirs("eval", exist_ok=True)
    p = jeval.build_parser()
    assert p.parse_args([]).cut_last == 0 and p.parse_args(["--cut_last", "2"]).cut_last == 2
    best, nbest, miss = jeval.main(["-e", "1", "-es", "8", "-b", "5", "--batch", "4", "--cut_last", "1"])
    assert best + nbest + miss == 8
    assert "cut_last 1 pred_best_hit %d pred_nbest_hit %d pred_miss %d eval_size 8" % (best, nbest, miss) in capsys.readouterr().out
    (name,) = os.listdir("eval")
    assert name.endswith("_cut_1.txt")
    with open(os.path.join("eval", name), encoding="utf-8") as fh:
        body = fh.read()
    assert body.count("hit\n") == 8
    for bad in (["-vs", "1"], ["-dd", "1"], ["-ng", "1"]):
        with pytest.raises(ValueError):
            jeval.Evaluator(p.parse_args(["-e", "1", "--cut_last", "1"] + bad))


def test_command_line_prints_both_lists(fake, capsys):
    from jlm_amd import complete
    text = pc.inputs()[4]
    cc.set_root("tied")
    res = complete.main(["--root", cc.model_root("tied"), "-e", "1", "--convert", text, "-b", "5", "--n-best", "4"])
    out = capsys.readouterr().out.splitlines()
    out = out[out.index("conversions:"):]                # (the model's load line comes first)
    (conv, pred), = res
    assert out[0] == "conversions:" and out[1 + len(conv)] == "predictions:" and len(out) == 2 + len(conv) + len(pred)
    assert len(pred) == 4 and len(conv) <= 4
    assert out[2 + len(conv)].split("\t")[0] == " ".join(w.split("/")[0] for w in pred[0][1])
    with pytest.raises(SystemExit):
        complete.main(["--root", cc.model_root("tied"), "-e", "1", "--convert", text, "--top", "3"])
