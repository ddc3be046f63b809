"""GPU: prediction and completion under the n-gram mixture end to end (the ``ngram=`` of LSTM_Model.predict_top / predict_reading /
complete / complete_reading; csrc jlm_complete_frames_ngram, ngram_mix_rows_kernel, ngram_hist_advance_kernel) on the five models of
tests/test_gpu_cache.py, orders 2 and 3, beams 1 / 5 / 17: the lists against the oracle's mixed logits, the beams against the oracle
followed on the device's own parents (tests/ngram_mix_cases.py: tests/test_gpu_complete.py's bars plus the derived n-gram bar), a table
that does not sum to one, ``ngram=None`` giving what the call gave before, and no result depending on what the call's buffers held."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import ngram_mix_cases as nc, poison                                          # noqa: E402
from tests.gpu_rows import fixture_model, oracle_lm                                       # noqa: E402
from tests.test_gpu_cache import MODELS                                                   # noqa: E402

pytestmark = pytest.mark.gpu

BEAMS = (1, 5, 17)


def cases(model, seed=4):
    """-> (mix factory by order, prompts over the table's words, kana prefixes and their word sets)"""
    V = model.dev.V
    x, y = nc.stream(V, seed=seed)
    words = np.unique(x)
    rng = np.random.RandomState(8)
    prompts = [[nc.EOS] + [int(w) for w in words[rng.randint(0, len(words), size=k)]] for k in (2, 0, 1, 4, 3, 1)]
    index = model.reading_index()
    kana = [index.readings[int(np.flatnonzero(index.ids == int(words[i]))[0])][:1] for i in range(len(prompts))]
    return (lambda order: nc.stream_table(x, y, V, order)), prompts, kana, [index.lookup(r) for r in kana]


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("name", MODELS)
def test_predictions_and_beams_against_the_oracle(name, order, fx, monkeypatch):
    f, model = fixture_model(fx, name, monkeypatch)
    lm = oracle_lm(f["root"])
    table_of, prompts, kana, sets = cases(model)
    mix = table_of(order)
    plain = model.predict_top(prompts, n=17)
    exact = 0
    for n in BEAMS:
        top = model.predict_top(prompts, n=n, ngram=mix)
        exact += nc.check_top(top, lm, mix, prompts, n, tag="%s top %d" % (name, n))
        rd = model.predict_reading(prompts, kana, n=n, ngram=mix)
        exact += nc.check_top(rd, lm, mix, prompts, n, sets=sets, tag="%s reading %d" % (name, n))
    assert exact >= 100, exact
    # the table moves the lists (a self-normalised fixture's logits are not normalised -- random weights --, and may outweigh it: there
    # every log p still moves, by log(1 - lam) at the least)
    mixed = model.predict_top(prompts, n=17, ngram=mix)
    assert all(not np.array_equal(a[1], b[1]) for a, b in zip(mixed, plain))
    assert lm.config["self_norm"] or any(not np.array_equal(a[0], b[0]) for a, b in zip(mixed, plain))
    comp = model._completer()
    N = 3
    order_p = np.argsort(-np.array([len(p) for p in prompts]), kind="stable")
    sorted_prompts = [np.asarray(prompts[i]) for i in order_p]
    shift = -np.log1p(-float(np.float32(mix.lam))) if lm.config["self_norm"] else 0.0
    for B in BEAMS:
        bp_parent, bp_word, bp_nll, score = comp.run(sorted_prompts, N, B, ngram=mix)
        agree = amb = 0
        for p, i in enumerate(order_p):
            a, b = nc.oracle_follow(lm, mix, prompts[i], bp_parent, bp_word, bp_nll, score, p, N, B)
            agree, amb = agree + a, amb + b
        assert amb <= max(1, (agree + amb) // 20), (name, B, agree, amb)
        res = model.complete(prompts, N, beam_width=B, ngram=mix)
        for p, i in enumerate(order_p):
            assert len(res[i]) == B and [h[2] for h in res[i]] == sorted(h[2] for h in res[i])
            for r, (ids, nll, tot) in enumerate(res[i]):
                assert len(ids) == N and abs(tot - (score[p * B + r] + N * shift)) <= 1e-9 and abs(nll.sum() - tot) <= 1e-9
    # the first word inside a reading's set, the later words free: the masked first frame under the mixture
    bp_parent, bp_word, bp_nll, score = comp.run(sorted_prompts, 2, 5, first_sets=[sets[i] for i in order_p], ngram=mix)
    for p, i in enumerate(order_p):
        if len(sets[i]) > 5:
            nc.oracle_follow(lm, mix, prompts[i], bp_parent, bp_word, bp_nll, score, p, 2, 5, first_set=sets[i])
    for r, S in zip(model.complete_reading(prompts, kana, 2, beam_width=5, ngram=mix), sets):
        assert r and all(int(h[0][0]) in set(S.tolist()) for h in r)


def test_stop_id_and_a_table_that_does_not_sum_to_one(fx, monkeypatch):
    f, model = fixture_model(fx, "small-vtable", monkeypatch)
    lm = oracle_lm(f["root"])
    table_of, prompts, _kana, _sets = cases(model)
    leaky = nc.leaky_table(table_of(3), model.dev.V)
    for n in (1, 5):
        nc.check_top(model.predict_top(prompts, n=n, ngram=leaky), lm, leaky, prompts, n, tag="leaky")
    mix = table_of(3)
    res = model.complete(prompts, 5, beam_width=5, ngram=mix)
    stop = int(np.bincount(np.concatenate([h[0][:2] for r in res for h in r])).argmax())      # a word the beams reach early
    order_p = np.argsort(-np.array([len(p) for p in prompts]), kind="stable")
    bp_parent, bp_word, bp_nll, score = model._completer().run([np.asarray(prompts[i]) for i in order_p], 5, 5, stop, ngram=mix)
    for p, i in enumerate(order_p):
        nc.oracle_follow(lm, mix, prompts[i], bp_parent, bp_word, bp_nll, score, p, 5, 5, stop_id=stop)
    res2 = model.complete(prompts, 5, beam_width=5, stop_id=stop, ngram=mix)
    assert any(len(h[0]) < 5 for r in res2 for h in r) and all(h[0][-1] == stop for r in res2 for h in r if len(h[0]) < 5)


@pytest.mark.parametrize("name", ["small-tied", "odd-tied"])
def test_ngram_none_is_the_call_it_was_and_no_buffer_matters(name, fx, monkeypatch):
    f, model = fixture_model(fx, name, monkeypatch)
    table_of, prompts, kana, sets = cases(model)
    mix = table_of(3)
    for a, b in zip(model.predict_top(prompts, n=5), model.predict_top(prompts, n=5, ngram=None)):
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    for ra, rb in zip(model.complete(prompts, 3, beam_width=4), model.complete(prompts, 3, beam_width=4, ngram=None)):
        assert poison.bits([list(h) for h in ra]) == poison.bits([list(h) for h in rb])

    def call():
        return [[list(h) for h in r] for r in model.complete(prompts, 3, beam_width=4, ngram=mix)] + \
               [list(t) for t in model.predict_reading(prompts, kana, n=4, ngram=mix)]
    poison.assert_same_three(call, what="complete(ngram=)")


def test_refusals(fx, monkeypatch):
    f, model = fixture_model(fx, "small-tied", monkeypatch)
    table_of, prompts, kana, _sets = cases(model)
    mix = table_of(3)
    for bad in (mix.table, "mix", 0.5):
        with pytest.raises(ValueError):
            model.predict_top(prompts, n=3, ngram=bad)
        with pytest.raises(ValueError):
            model.predict_reading(prompts, kana, n=3, ngram=bad)
        with pytest.raises(ValueError):
            model.complete(prompts, 2, beam_width=3, ngram=bad)
        with pytest.raises(ValueError):
            model.complete_reading(prompts, kana, 2, beam_width=3, ngram=bad)


def test_complete_command_line_with_ngram(fx, capsys, tmp_path):
    """--ngram FILE --ngram-lam L: --top prints predict_top(ngram=)'s list, completions complete(ngram=)'s"""
    from jlm_amd import complete as comp_mod, config as jconfig
    from jlm_amd.data import Vocab
    from jlm_amd.ngram import NGramMix, NGramTable, estimate, write_srilm
    from tests.gpu_rows import load_model
    f = fx("small-vtable")
    jconfig.set_root(f["root"])
    vocab = Vocab(f["cfg"]["vocab_size"])
    lex = f["lexicon"]
    prompt = " ".join(w for w, _c in lex[3:5])
    ids = [vocab.w2i[w] for w, _c in lex[3:9]]
    lm_path = str(tmp_path / "lm3")
    write_srilm(estimate(np.array((ids + [nc.EOS]) * 6), len(vocab), 3, eos=nc.EOS).rounded(), lm_path, vocab.i2w)
    lines = lambda: [l for l in capsys.readouterr().out.split("\n") if l and not l.startswith("LSTM model:")]
    base = ["--root", f["root"], "-e", "1", "--prompt", prompt]
    plain = comp_mod.main(base + ["--top", "5"])
    lines()
    res = comp_mod.main(base + ["--top", "5", "--ngram", lm_path, "--ngram-lam", "0.5"])
    out = lines()
    model = load_model(f["root"])
    mix = NGramMix(NGramTable.from_srilm(lm_path, vocab.t2i, 3), 0.5)
    want = model.predict_top([[nc.EOS] + ids[:2]], n=5, ngram=mix)
    assert len(out) == 5 and np.array_equal(res[0][0], want[0][0]) and res[0][1].tobytes() == want[0][1].tobytes()
    assert res[0][0][0] == ids[2] and not np.array_equal(res[0][1], plain[0][1])          # the passage's next word leads the list
    res = comp_mod.main(base + ["--words", "3", "-b", "4", "--ngram", lm_path, "--ngram-lam", "0.5", "--ngram-order", "2"])
    assert len(lines()) == 4 and len(res[0]) == 4
    mix2 = NGramMix(NGramTable.from_srilm(lm_path, vocab.t2i, 2), 0.5)
    for a, b in zip(res[0], model.complete([[nc.EOS] + ids[:2]], 3, beam_width=4, ngram=mix2)[0]):
        assert np.array_equal(a[0], b[0]) and a[2] == b[2]
    for bad in (["--ngram", lm_path], ["--ngram-lam", "0.5"], ["--ngram", lm_path, "--ngram-lam", "1.0"],
                ["--ngram", lm_path, "--ngram-lam", "0.5", "--ngram-order", "4"], ["--ngram", lm_path, "--ngram-lam", "0.5", "--convert", "a"]):
        with pytest.raises(SystemExit):
            comp_mod.main(base + bad)
