"""CPU: the n-gram mixture in decode -- the yardstick checks itself (tests/decode_ngram_cases.py), the
estimator, the file format and the hash table (jlm_amd/ngram.py), every refusal, the host-side search against the proxy, and the
command-line flags."""
import types

import numpy as np
import pytest

from jlm_amd import context as jctx
from jlm_amd.model_ngram import NGramModel
from jlm_amd.ngram import NGramMix, NGramTable, check_mix, estimate, pack, write_srilm
from tests import context_cases as cc
from tests import decode_ngram_cases as nc
from tests import fake_hip, fake_ngram
from tests.decode_ngram_budget import score_bar


# ---------------------------------------------------------------------------------------------- the yardstick checks itself
@pytest.mark.parametrize("order", nc.ORDERS)
@pytest.mark.parametrize("name", ["tied", "vtable", "tied-h512"])
def test_mixed_oracle_is_the_chain_rule_and_moves_the_result(name, order):
    """the proxy's 1-best score = the chain-rule sum of -log p_mix along its path, to 1e-9; with the chosen corpus and lambda the mixed
    oracle's 1-best differs from the plain oracle's on at least 4 of the 12 inputs, and on every input the two top scores differ by
    more than twice the GPU test's bar -- the fixture cannot degenerate silently"""
    o, mix = cc.oracle(name), nc.mix(name, order)
    moved = 0
    for k, (text, ctx) in enumerate(zip(nc.sentences(), nc.contexts(name))):
        for c in (None, ctx):
            got = nc.mixed_decode(o, text, c, mix, beam_width=5)
            score, words = got[0]
            want = nc.chain_nll_mix(o.model, [cc.EOS] + cc.ids_of(c), cc.path_ids(o, words), mix).sum()
            assert abs(score - want) <= 1e-9, (name, order, text, c, score, want)
            plain = cc.primed_decode(o, text, c, beam_width=5)
            moved += (c is None) and got[0][1] != plain[0][1]
            assert abs(score - plain[0][0]) > 2 * score_bar(score, len(words)), (name, order, text, c, score, plain[0][0])
    assert moved >= 4, moved


def test_ngram_lm_is_the_definition():
    o, mix = cc.oracle("tied"), nc.mix("tied", 3)
    ctx = [7, 9]
    p = nc.NGramLM(o.model, [cc.EOS] + ctx, mix)
    h, c = p.zero_state(1)
    pred, _y, h2, c2, _a, _b = p.predict([cc.EOS], h, c)
    plain = o.model.predict([9], h, c)[0]
    q = np.array([mix.table.logq([7, 9], w) for w in range(plain.shape[1])])
    np.testing.assert_allclose(pred[0], (1 - mix.lam) * plain[0] + mix.lam * np.exp(q), rtol=1e-12, atol=0)
    assert abs(pred.sum() - 1.0) < 1e-6                                    # (the rounded table: float32 values)
    pred2 = p.predict([11], h2, c2)[0]
    q = np.array([mix.table.logq([9, 11], w) for w in range(plain.shape[1])])
    np.testing.assert_allclose(pred2[0], (1 - mix.lam) * o.model.predict([11], h2, c2)[0][0] + mix.lam * np.exp(q), rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------- the estimator, the file, the table
def _stream(V, seed, n=300):
    rng = np.random.RandomState(seed)
    ids = []
    for _ in range(n):
        ids += [int(x) for x in np.minimum(rng.geometric(0.15, size=rng.randint(1, 9)) + 1, V - 1)] + [cc.EOS]
    return ids


@pytest.mark.parametrize("order", [1, 2, 3])
def test_estimated_tables_sum_to_one(order):
    V = 40
    table = estimate(_stream(V, 3), V, order)
    rng = np.random.RandomState(order)
    for _ in range(50):
        h = [int(x) for x in rng.randint(0, V, size=rng.randint(0, 5))]
        total = sum(np.exp(table.logq(h, w)) for w in range(V))
        assert abs(total - 1.0) <= 1e-9, (order, h, total)
        assert abs(np.exp(table.logq_all(h, V)).sum() - 1.0) <= 1e-9
        np.testing.assert_array_equal(table.logq_all(h, V), [table.logq(h, w) for w in range(V)])


def _vocab(V):
    i2w = {i: "w%d/r%d/x" % (i, i) for i in range(V)}
    i2w[0], i2w[1] = "<unk>", "<eos>"
    return i2w, {w: i for i, w in i2w.items()}


def test_write_srilm_round_trip(tmp_path, capsys):
    V = 40
    i2w, w2i = _vocab(V)
    table = estimate(_stream(V, 5), V, 3).rounded()
    path = str(tmp_path / "lm3")
    write_srilm(table, path, i2w)
    back = NGramTable.from_srilm(path, w2i, 3)
    a, b = table.device_arrays(), back.device_arrays()
    assert a["keys"].tobytes() == b["keys"].tobytes() and a["vals"].tobytes() == b["vals"].tobytes()
    assert (a["log2cap"], a["max_probe"]) == (b["log2cap"], b["max_probe"])
    # the existing reader gives the same costs
    old = NGramModel.parse_srilm(object.__new__(NGramModel), path)
    assert len(old) == len(table)
    for key, lp, bow in zip(table.keys.tolist(), table.lp.tolist(), table.bow.tolist()):
        ids = [x for x in (((key >> sh) & 0x1FFFFF) - 1 for sh in (42, 21, 0)) if x >= 0]
        cost, backoff = old[tuple(i2w[x] for x in ids)]
        assert abs(cost + lp) <= 1e-12 * max(1.0, abs(lp))
        assert (backoff is None and bow == 0.0) or abs(backoff + bow) <= 1e-12 * max(1.0, abs(bow))
    # a lower order reads the file's shorter n-grams only
    two = NGramTable.from_srilm(path, w2i, 2)
    assert two.order == 2 and len(two) == int((table.keys < (1 << 42)).sum())


def test_sentence_marks_merge(tmp_path):
    _i2w, w2i = _vocab(6)
    path = tmp_path / "lm"
    path.write_text("\n\\data\\\nngram 1=4\n\n\\1-grams:\n-99\t<s>\t-0.5\n-1.25\t</s>\n-0.75\tw2/r2/x\t-0.25\n-2\tnot-a-word\n"
                    "\n\\2-grams:\n-0.5\t<s> w2/r2/x\n-0.25\tw2/r2/x </s>\n-3\tw2/r2/x not-a-word\n\n\\end\\\n", encoding="utf-8")
    t = NGramTable.from_srilm(str(path), w2i, 3)
    ln10 = np.log(10.0)
    f32 = lambda x: float(np.float32(ln10 * x))
    assert len(t) == 4                                                     # the two forms of <eos> merged, unknown words dropped
    assert t.entry([1]) == (f32(-1.25), f32(-0.5))                         # lp from </s>, bow from <s>: -99 is no probability
    assert t.entry([2]) == (f32(-0.75), f32(-0.25))
    assert t.entry([1, 2]) == (f32(-0.5), 0.0) and t.entry([2, 1]) == (f32(-0.25), 0.0)
    assert t.logq([1], 2) == f32(-0.5) and t.logq([3], 2) == f32(-0.75)   # an unseen context: no weight
    assert t.logq([2], 2) == f32(-0.25) + f32(-0.75) and t.logq([2], 3) == -np.inf
    # the other order of the two forms gives the same table
    path.write_text("-1.25\t</s>\n-99\t<s>\t-0.5\n", encoding="utf-8")
    assert NGramTable.from_srilm(str(path), w2i, 1).entry([1]) == (f32(-1.25), f32(-0.5))


def test_hash_table_looks_up_as_a_dict():
    V = 60
    table = estimate(_stream(V, 7, n=400), V, 3).rounded()
    want = {int(k): (float(np.float32(lp)), float(np.float32(bow))) for k, lp, bow in zip(table.keys, table.lp, table.bow)}
    rng = np.random.RandomState(1)
    absent = set()
    while len(absent) < 1000:
        k = pack([int(x) for x in rng.randint(0, V + 5, size=rng.randint(1, 4))])
        if k not in want:
            absent.add(k)
    for kw in ({}, dict(min_log2cap=14), dict(log2cap=int(np.floor(np.log2(2 * len(table)))))):
        arr = table.device_arrays(**kw)
        cap = 1 << arr["log2cap"]
        assert arr["keys"].shape == (cap,) and arr["keys"].dtype == np.uint64 and arr["vals"].shape == (cap, 2) and arr["vals"].dtype == np.float32
        assert cap >= 64 and int((arr["keys"] != 0).sum()) == len(table)
        if not kw:
            assert cap >= 2 * len(table) > cap // 2
        for k, v in want.items():
            assert fake_ngram.probe(arr, k) == v
        for k in absent:
            assert fake_ngram.probe(arr, k) is None
        assert arr["keys"].tobytes() == NGramTable(table.keys[::-1], table.lp[::-1], table.bow[::-1], 3).device_arrays(**kw)["keys"].tobytes()
    assert arr["max_probe"] >= 3 and 2 * len(table) >= cap                 # at a load of a half and more the probes walk
    # back-off over the hash table = the definition
    for _ in range(200):
        h = [int(x) for x in rng.randint(0, V, size=rng.randint(0, 4))]
        w = int(rng.randint(0, V + 3))
        for order in (1, 2, 3):
            sub = NGramTable(table.keys[table.keys < (1 << (21 * order))], table.lp[table.keys < (1 << (21 * order))],
                             table.bow[table.keys < (1 << (21 * order))], order)
            assert fake_ngram.logq(arr, order, h, w) == sub.logq(h, w)
    assert min(len(table), 1) and table.max_id == V - 1


def test_tables_refuse_what_the_kernel_has_no_flag_for():
    for keys, lp, bow, order in (([pack([1])], [0.5], [0.0], 1), ([pack([1])], [-np.inf], [0.0], 1), ([pack([1])], [-1.0], [np.nan], 1),
                                 ([pack([1, 2])], [-1.0], [0.0], 1), ([pack([1])], [-1.0], [0.0], 4), ([pack([1]), pack([1])], [-1.0, -2.0], [0, 0], 1)):
        with pytest.raises(ValueError):
            NGramTable(keys, lp, bow, order)
    with pytest.raises(ValueError):
        estimate([1, 2, 1], (1 << 21), 2)
    with pytest.raises(ValueError):
        estimate([1, 5, 1], 4, 2)
    t = NGramTable([pack([1])], [-1.0], [0.0], 1)
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            NGramMix(t, bad)
    with pytest.raises(ValueError):
        NGramMix("table", 0.5)
    with pytest.raises(ValueError):
        t.device_arrays(log2cap=5)


def test_patch_double_is_the_mixture():
    table = estimate(_stream(30, 2), 30, 3).rounded()
    arr = table.device_arrays()
    hists, words = [[1], [4, 5], [2, 1, 7]], [3, 0, 29]
    y = np.array([[-3.0, -1.0, -7.5], [-2.0, -9.0, -0.5], [-4.0, -4.0, -4.0]], dtype=np.float32)
    L = np.array([0.25, -0.5, 1.5])
    got = fake_ngram.patch_cell(arr, 3, 0.5, hists, words, y, L)
    for p, w in enumerate(words):
        for k, h in enumerate(hists):
            prob = 0.5 * np.exp(float(y[p, k]) - L[k]) + 0.5 * np.exp(table.logq(h, w))
            assert abs(float(got[p, k]) - (L[k] + np.log(prob))) <= 2.0 ** -24 * abs(L[k] + np.log(prob)) + 1e-12


# ---------------------------------------------------------------------------------------------- the decoders
@pytest.fixture()
def decoder(monkeypatch):
    fake_hip.install(monkeypatch)
    cc.set_root("tied")
    from jlm_amd.decoder import Decoder
    d = Decoder(1)
    d.perf_timing = False
    return d


class _HostState(jctx.ContextState):
    """a ContextState whose host copies are given (no device): what the host-side searches read"""

    def __init__(self, m, host, tails=None):
        self.m, self.n = m, len(host)
        self.last_host = np.asarray([x[2] for x in host], dtype=np.int32)
        self.has_host = np.ones(self.n, dtype=np.int32)
        self.tail_host = np.asarray(tails if tails is not None else [[-1, x[2]] for x in host], dtype=np.int32)
        self._host = host

    def numpy(self):
        return np.concatenate([x[0] for x in self._host]), np.concatenate([x[1] for x in self._host])


def _host_state(d, o, ctxs):
    host, tails = [], []
    for c in ctxs:
        hist = [cc.EOS] + list(c)
        h, cl = cc.oracle_state(o.model, hist[:-1])
        host.append((h.astype(np.float32), cl.astype(np.float32), hist[-1]))
        tails.append(([-1] + hist)[-2:])
    return _HostState(d.model.dev, host, tails)


@pytest.mark.parametrize("order", nc.ORDERS)
def test_host_search_under_the_mixture_equals_the_proxy(decoder, order):
    """beam_width=None over the numpy ABI double: the unpruned host-side search mixes every frame's probabilities by the float64
    definition, with and without a left context"""
    d, o, mix = decoder, cc.oracle("tied"), nc.mix("tied", order)
    sents, ctxs = nc.sentences(), nc.contexts("tied")
    pick = [i for i in range(len(sents)) if cc.ids_of(ctxs[i]) and len(sents[i]) <= 4][:3]
    texts = [sents[i] for i in pick]
    state = _host_state(d, o, [cc.ids_of(ctxs[i]) for i in pick])
    plain = d.decode_batch(texts, beam_width=None)
    assert d.decode_batch(texts, beam_width=None, ngram=None) == plain
    for context, cs in ((None, [None] * len(pick)), (state, [ctxs[i] for i in pick])):
        got = d.decode_batch(texts, beam_width=None, context=context, ngram=mix)
        for text, c, g, p in zip(texts, cs, got, plain):
            want = nc.mixed_decode(o, text, c, mix, beam_width=None)
            assert [w for _, w in g] == [w for _, w in want]
            np.testing.assert_allclose([x for x, _ in g], [x for x, _ in want], rtol=2e-6, atol=2e-5)
            assert [x for x, _ in g] != [x for x, _ in p]


def test_a_state_without_a_tail_counts_as_its_last_word():
    s = jctx.ContextState(None, None, None, None, None, [1, 4], [0, 1])
    assert s.tail_host.tolist() == [[-1, 1], [-1, 4]]
    s = jctx.ContextState(None, None, None, None, None, [1, 4], [0, 1], tail_host=[[-1, 1], [9, 4]])
    assert s.tail_host.tolist() == [[-1, 1], [9, 4]] and jctx.DecodeContext(s, [1, 0]).tail(0) == [9, 4]
    assert jctx.DecodeContext(s, [1, 0]).tail(1) == [1]


def test_refusals_before_anything_runs(decoder):
    d, o = decoder, cc.oracle("tied")
    mix = nc.mix("tied", 3)
    text = nc.sentences()[1]
    from jlm_amd.cache import CacheSpec
    spec = CacheSpec(16, theta=0.5, lam=0.5)
    d.model._primer = lambda: pytest.fail("primed")
    d._engine.submit = lambda *a, **k: pytest.fail("submitted")
    cached = object.__new__(jctx.CachedContext)
    V = len(d.w2i)
    big = NGramMix(NGramTable([pack([V])], [-1.0], [0.0], 1), 0.5)
    for call in (lambda: d.decode(text, context=[5, 6], cache=spec, ngram=mix),
                 lambda: d.decode_batch([text], context=cached, ngram=mix),
                 lambda: d.decode(text, vocab_select=True, ngram=mix),
                 lambda: d.decode_predict(text, ngram=mix),
                 lambda: d.decode_predict_batch([text], ngram=mix),
                 lambda: d.decode(text, ngram=big),
                 lambda: d.decode(text, ngram=mix.table),
                 lambda: d.decode(text, ngram=0.5),
                 lambda: d.decode(text, beam_width=None, ngram="lm3")):
        with pytest.raises(ValueError):
            call()
    d.compat_quirks = True
    with pytest.raises(ValueError):
        d.decode(text, ngram=mix)
    d.compat_quirks = False
    from jlm_amd import shard
    with pytest.raises(ValueError):
        shard.decode_sharded(d, [text], 0, 1, ngram=mix)
    from jlm_amd.decoder_dynamic import DynamicDecoder
    dd = DynamicDecoder(1)
    with pytest.raises(ValueError):
        dd.decode(text, vocab_select=True, ngram=mix)
    from jlm_amd.decoder_char import CharRNNDecoder
    from jlm_amd.decoder_ngram import NGramDecoder
    for cls in (CharRNNDecoder, NGramDecoder):
        with pytest.raises(ValueError):
            cls.decode(object.__new__(cls), text, ngram=mix)
    assert check_mix(mix, V) is mix
    # the engine refuses on its own too
    from jlm_amd.engine import DecodeEngine
    eng = object.__new__(DecodeEngine)
    eng.m, eng.torch = types.SimpleNamespace(V=V), None
    lat = types.SimpleNamespace(n_nodes=1, max_cands=1, n_sent=1)
    with pytest.raises(ValueError):
        DecodeEngine._submit(eng, lat, "static", (np.zeros(1), np.zeros(2)), None, 10, False, ngram=mix)
    with pytest.raises(ValueError):
        DecodeEngine._submit(eng, lat, "static", None, None, 10, False, ngram=big)


# ---------------------------------------------------------------------------------------------- the command-line tools
def test_eval_flags_and_log_name():
    from jlm_amd import eval as jeval
    p = jeval.build_parser()
    a = p.parse_args([])
    assert a.ngram_mix is None and a.ngram_lam == 0.3 and a.ngram_order == 3
    assert sorted(vars(a)) == sorted(["experiment_id", "eval_size", "use_ngram", "ngram_order", "comp", "vocab_select", "top_sampling",
                                      "random_sampling", "samples", "beam_size", "dynamic_decoding", "root", "batch", "context_words",
                                      "cache", "theta", "lam", "cut_last", "ngram_mix", "ngram_lam"])
    a = p.parse_args(["--ngram_mix", "lm3", "--ngram_lam", "0.2", "--ngram_order", "2"])
    assert (a.ngram_mix, a.ngram_lam, a.ngram_order) == ("lm3", 0.2, 2)
    ev = object.__new__(jeval.Evaluator)
    ev.args, ev.context_words, ev.cut_last, ev.cache = a, 0, 0, None
    plain = ev.log_name()                                                  # without the flag the name is what it was
    ev.ngram_mix = None
    assert ev.log_name() == plain and "ngmix" not in plain
    ev.ngram_mix = NGramMix(NGramTable([pack([1])], [-1.0], [0.0], 2), 0.2)
    assert ev.log_name() == plain[:-len(".txt")] + "_ngmix_2.txt"


def test_perplexity_of_the_mixture(tmp_path, capsys):
    from jlm_amd import perplexity as pp
    from jlm_amd.ngram import mixture_nll
    nll, logq = np.array([1.0, 2.0, 0.5]), np.array([-0.5, -np.inf, -3.0])
    for lam in (0.1, 0.5):
        want = -np.log((1 - lam) * np.exp(-nll) + lam * np.exp(logq))
        np.testing.assert_allclose(mixture_nll(nll, logq, lam), want, rtol=1e-14)
        assert abs(pp.ngram_mixture_perplexity(nll, logq, lam) - np.exp(want.mean())) <= 1e-12
    # the scores of a stream: the model's -log p as score_streams returns it, q from the table over each row's own words
    V = 12
    table = estimate(_stream(V, 4, n=50), V, 3).rounded()
    stream = _stream(V, 9, n=20)
    model = types.SimpleNamespace(score_streams=lambda x, y, h, c: (np.full(np.shape(x), 2.0), h, c))
    got_nll, got_q = pp.stream_ngram_scores(model, stream, 3, 5, table)
    from jlm_amd.score import stream_layout
    x, y = stream_layout(stream, 3, 5)
    T = x.shape[1] // 5 * 5
    assert got_nll.shape == got_q.shape == (3 * T,) and (got_nll == 2.0).all()
    q = got_q.reshape(3, T)
    assert q[1, 0] == table.logq([x[1, 0]], y[1, 0]) and q[2, 4] == table.logq([x[2, 3], x[2, 4]], y[2, 4])
    # the flags are refused where they mean nothing
    for argv in (["--tune-ngram", "dev.txt"], ["--ngram", "lm3", "--mode", "sentence"], ["--ngram", "lm3", "--ngram-lam", "1.5"]):
        with pytest.raises(SystemExit):
            pp.main(argv)
    capsys.readouterr()


def test_cli_writes_the_file_the_baseline_reads(tmp_path, capsys):
    from jlm_amd import config as jconfig, ngram as jng, synth
    root = str(tmp_path)
    V = 50
    synth.write_lexicon(root, V, alphabet=cc.ALPHABET)
    jconfig.set_root(root)
    from jlm_amd.data import Vocab
    vocab = Vocab(V)
    rng = np.random.RandomState(0)
    import os
    with open(os.path.join(jconfig.data_path, "train.txt"), "w", encoding="utf-8") as f:
        for _ in range(40):
            f.write(" ".join(vocab.i2w[int(i)] for i in rng.randint(2, V, size=rng.randint(1, 6))) + "\n")
    assert jng.main(["--root", root, "--vocab_size", str(V), "--order", "3"]) == 0
    out = os.path.join(jconfig.data_path, "lm3")
    table = NGramTable.from_srilm(out, vocab.w2i, 3)
    assert len(table) > V and abs(sum(np.exp(table.logq([cc.EOS], w)) for w in range(len(vocab))) - 1.0) < 1e-5
    model = NGramModel("lm3", 3)                                           # the baseline reads the same file
    assert len(model.model) == len(table)
    capsys.readouterr()
