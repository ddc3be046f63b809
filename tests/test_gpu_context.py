"""GPU: decoding with a left context (Decoder.decode / decode_batch(context=), LSTM_Model.prime; csrc jlm_prime_frames,
seed_context_kernel, frame 0 of jlm_decode_frames) against the UNMODIFIED oracle behind the proxy of tests/context_cases.py.

Bars: those of tests/random_models.check against the primed oracle (equal list lengths, identical 1-best words, every score within
rtol 2e-6 / atol 2e-5); the decode suite's 1e-6 per frame (+ 2e-6) between a path's score and the device's own chain rule
(LSTM_Model.score); rtol 1e-4 / atol 1e-5 (the predict API's) on the primed state; bit equality wherever two calls must enqueue the
same launches, and for the rows the seeding kernel gathers."""
import contextlib
import io
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib, config as jconfig, synth      # noqa: E402
from tests import context_cases as cc                   # noqa: E402

pytestmark = pytest.mark.gpu

SENTS = cc.sentences()
_DEC = {}


def decoder(name, dynamic=False):
    """the model's decoder, loaded once for the module"""
    key = (name, dynamic)
    if key not in _DEC:
        cc.set_root(name)
        from jlm_amd.decoder import Decoder
        from jlm_amd.decoder_dynamic import DynamicDecoder
        _DEC[key] = (DynamicDecoder if dynamic else Decoder)(1)
    return _DEC[key]


def ctxs_of(name):
    return cc.contexts(cc.MODELS[name][0])


# ---------------------------------------------------------------------------------------------- against the primed oracle
# (an untied projection has no vocabulary subset: reference model.py:189)
@pytest.mark.parametrize("name,select", [(n, s) for n in cc.MODELS for s in (False, True) if not (s and n == "untied")])
def test_static_against_primed_oracle(name, select):
    d, o, ctxs = decoder(name), cc.oracle(name), ctxs_of(name)
    kw = dict(vocab_select=True) if select else {}
    for beam in cc.BEAMS:
        got = d.decode_batch(SENTS, beam_width=beam, context=ctxs, **kw)
        for s, c, g in zip(SENTS, ctxs, got):
            cc.check_nbest(g, cc.primed_decode(o, s, c, beam_width=beam, **kw), (name, select, beam, s, c))
    # the single-sentence entry point, ids and lexicon strings alike
    i = 4
    want = cc.primed_decode(o, SENTS[i], ctxs[i], beam_width=5, **kw)
    cc.check_nbest(d.decode(SENTS[i], beam_width=5, context=ctxs[i], **kw), want, (name, "decode"))
    cc.check_nbest(d.decode(SENTS[i], beam_width=5, context=[o.i2w[w] for w in cc.ids_of(ctxs[i])], **kw), want, (name, "strings"))


@pytest.mark.parametrize("name", cc.TIED)
def test_dynamic_against_primed_oracle(name):
    d, o, ctxs = decoder(name, dynamic=True), cc.oracle(name, dynamic=True), ctxs_of(name)
    for beam in cc.BEAMS:
        got = d.decode_batch(SENTS, beam_width=beam, vocab_select=True, context=ctxs)
        for s, c, g in zip(SENTS, ctxs, got):
            cc.check_nbest(g, cc.primed_decode(o, s, c, beam_width=beam, vocab_select=True), (name, "dynamic", beam, s, c))


def test_context_changes_the_result():
    d = decoder("tied")
    plain = d.decode_batch(SENTS, beam_width=5)
    with_ctx = d.decode_batch(SENTS, beam_width=5, context=ctxs_of("tied"))
    assert sum(a != b for a, b in zip(plain, with_ctx)) >= 8


# ---------------------------------------------------------------------------------------------- the chain rule on the device
@pytest.mark.parametrize("name", list(cc.MODELS))
def test_chain_rule_on_the_device(name):
    """every returned path's score = the tail of LSTM_Model.score([context + path], start=<eos>), 1e-6 per frame"""
    d, ctxs = decoder(name), ctxs_of(name)
    got = d.decode_batch(SENTS, beam_width=5, context=ctxs)
    seqs, meta = [], []
    for s, c, res in zip(SENTS, ctxs, got):
        for score, words in res:
            ids = [d.w2i.get(w, 0) for w in words]
            seqs.append(cc.ids_of(c) + ids)
            meta.append((s, score, len(ids)))
    nll = d.model.score(seqs, cc.EOS)
    for (s, score, n), tok in zip(meta, nll):
        bar = 1e-6 * (len(s) + 1) + 2e-6
        print(name, s, score, float(tok[len(tok) - n:].sum()), bar)
        assert abs(score - float(tok[len(tok) - n:].sum())) <= bar, (name, s, score, tok)


# ---------------------------------------------------------------------------------------------- empty contexts, reuse
@pytest.mark.parametrize("name,dynamic", [("tied", False), ("vtable", False), ("tied", True)])
def test_empty_contexts_are_todays_decode(name, dynamic):
    d = decoder(name, dynamic)
    kw = dict(beam_width=5, vocab_select=True) if dynamic else dict(beam_width=5)
    plain = d.decode_batch(SENTS, **kw)
    ctx_plans = lambda: sum(len(p.key) > 7 for p in d._engine.plans)
    before = ctx_plans()
    assert d.decode_batch(SENTS, context=[[]] * len(SENTS), **kw) == plain
    assert d.decode_batch(SENTS, context=[None] * len(SENTS), **kw) == plain
    assert d.decode_batch(SENTS, context=d.model.prime([[]] * len(SENTS)), **kw) == plain
    assert ctx_plans() == before                           # no plan with context rows was made: the launches of a call without context
    assert d.decode(SENTS[2], context=[], **kw) == d.decode(SENTS[2], **kw)


@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_reusing_a_primed_state(name, monkeypatch):
    d, ctxs = decoder(name), ctxs_of(name)
    state = d.model.prime([cc.ids_of(c) for c in ctxs])
    perm = np.random.RandomState(9).permutation(len(SENTS)).tolist()
    shuffled = [SENTS[i] for i in perm]
    assert d.decode_batch(shuffled, beam_width=5, context=state) == d.decode_batch(shuffled, beam_width=5, context=ctxs)
    monkeypatch.setattr(d, "max_batch", 4)
    assert len(d._chunks(SENTS, 5)) >= 3
    chunked = d.decode_batch(SENTS, beam_width=5, context=state)
    assert chunked == d.decode_batch(SENTS, beam_width=5, context=ctxs)
    o = cc.oracle(name)
    for s, c, g in zip(SENTS, ctxs, chunked):
        cc.check_nbest(g, cc.primed_decode(o, s, c, beam_width=5), (name, "chunked", s, c))
    with pytest.raises(ValueError):
        d.decode_batch(SENTS[:3], beam_width=5, context=state)               # one row per input
    with pytest.raises(ValueError):
        d.decode_batch(SENTS, beam_width=5, context=ctxs[:3])
    with pytest.raises(ValueError):
        d.decode_batch(SENTS[:1], beam_width=5, context=[[cc.MODELS[name][0]]])


# ---------------------------------------------------------------------------------------------- fallback paths
SHORT = [s[:4] for s in SENTS[:6]]


@pytest.mark.parametrize("name,dynamic", [("tied", False), ("vtable", False), ("tied", True)])
def test_unpruned_search_with_context(name, dynamic):
    d, o, ctxs = decoder(name, dynamic), cc.oracle(name, dynamic), ctxs_of(name)
    ctxs = [ctxs[2], ctxs[1]] + ctxs[4:8]                   # the 40-word context and the one holding <eos> among them
    kw = dict(vocab_select=True) if dynamic else {}
    got = d.decode_batch(SHORT, beam_width=None, context=ctxs, **kw)
    for s, c, g in zip(SHORT, ctxs, got):
        cc.check_nbest(g, cc.primed_decode(o, s, c, beam_width=None, **kw), (name, dynamic, "unpruned", s, c))


@pytest.mark.parametrize("name,dynamic", [("vtable", False), ("tied", True)])
def test_oversized_cells_take_the_host_path_with_context(name, dynamic, monkeypatch):
    d, o, ctxs = decoder(name, dynamic), cc.oracle(name, dynamic), ctxs_of(name)
    from jlm_amd.lattice import BatchLattice
    lat = BatchLattice(d._builder, SENTS, 6)
    per = np.diff(np.asarray(lat.end_off)).reshape(lat.n_frames, lat.n_sent).max(axis=0) * 6
    limit = int(np.sort(per)[len(per) // 2])
    monkeypatch.setattr(type(d), "CAND_LIMIT", limit)
    assert 0 < int((per > limit).sum()) < len(SENTS)
    kw = dict(vocab_select=True) if dynamic else {}
    got = d.decode_batch(SENTS, beam_width=6, context=ctxs, **kw)
    for s, c, g in zip(SENTS, ctxs, got):
        cc.check_nbest(g, cc.primed_decode(o, s, c, beam_width=6, **kw), (name, dynamic, "oversized", s, c))


def test_empty_inputs_and_the_stale_vocabulary_path(monkeypatch):
    d, o, ctxs = decoder("tied"), cc.oracle("tied"), ctxs_of("tied")
    sents = ["", SENTS[5], "", SENTS[6]]
    c4 = [ctxs[4], ctxs[5], None, ctxs[6]]
    got = d.decode_batch(sents, beam_width=5, context=c4)
    assert got[0] == [(0.0, [])] and got[2] == [(0.0, [])]
    cc.check_nbest(got[1], cc.primed_decode(o, sents[1], c4[1], beam_width=5), "beside empty inputs")
    cc.check_nbest(got[3], cc.primed_decode(o, sents[3], c4[3], beam_width=5), "beside empty inputs")
    assert d.decode("", context=ctxs[4]) == [(0.0, [])]
    monkeypatch.setattr(d, "compat_quirks", True)
    monkeypatch.setattr(d, "lattice_vocab", [1, 2, 3])
    with pytest.raises(ValueError, match="left context"):
        d.decode_batch(SENTS[:2], beam_width=5, context=ctxs[4:6])


# ---------------------------------------------------------------------------------------------- the primed state
@pytest.mark.parametrize("name", list(cc.MODELS))
def test_primed_state_against_the_oracle(name):
    d, o, ctxs = decoder(name), cc.oracle(name), ctxs_of(name)
    for max_rows in (None, 5):
        state = d.model.prime([cc.ids_of(c) for c in ctxs], max_rows=max_rows)
        h, c = state.numpy()
        assert h.dtype == np.float32 and h.shape == (len(ctxs), cc.MODELS[name][1]) == c.shape
        for i, ctx in enumerate(ctxs):
            ids = cc.ids_of(ctx)
            assert int(state.last_host[i]) == ([cc.EOS] + ids)[-1] and bool(state.has_host[i]) == bool(ids)
            if ids:
                hw, cw = cc.oracle_state(o.model, [cc.EOS] + ids[:-1])
                np.testing.assert_allclose(h[i], hw[0], rtol=1e-4, atol=1e-5)
                np.testing.assert_allclose(c[i], cw[0], rtol=1e-4, atol=1e-5)
            else:
                assert not h[i].any() and not c[i].any()
        assert state.last.cpu().numpy().tolist() == state.last_host.tolist() and state.has.cpu().numpy().tolist() == state.has_host.tolist()
    with pytest.raises(ValueError):
        d.model.prime([[2], [cc.MODELS[name][0]]])
    with pytest.raises(ValueError):
        d.model.prime([[-1]])


def test_primed_state_odd_vocabulary(fx):
    """the priming loop on the V = 2 003 model cut at 501 / 1 203: contexts that end and pass through the first and last word of every
    segment, against the oracle's state at the bars above; calls of 1, 31, 32 and 33 contexts give the rows of a call of 64 at the same
    bars"""
    from tests.gpu_rows import load_model, oracle_lm
    f = fx("odd-vtable")
    model = load_model(f["root"])
    assert model.dev.V == 2003
    lm = oracle_lm(f["root"])
    rng = np.random.RandomState(41)
    edges = (0, 500, 501, 1202, 1203, 2002)
    ctxs = []
    for i in range(64):
        c = [int(x) for x in rng.randint(2, 2003, size=rng.randint(1, 7))]
        c[-1] = edges[i % 6]
        c[0] = edges[(i // 6) % 6] if len(c) > 1 else c[0]
        ctxs.append(c)
    ctxs[5] = []
    state = model.prime(ctxs)
    h, c = state.numpy()
    assert h.shape == (64, 64) == c.shape
    for i, ids in enumerate(ctxs):
        assert int(state.last_host[i]) == ([cc.EOS] + ids)[-1] and bool(state.has_host[i]) == bool(ids)
        if ids:
            hw, cw = cc.oracle_state(lm, [cc.EOS] + ids[:-1])
            np.testing.assert_allclose(h[i], hw[0], rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(c[i], cw[0], rtol=1e-4, atol=1e-5)
        else:
            assert not h[i].any() and not c[i].any()
    for n in (1, 31, 32, 33):
        hn, cn = model.prime(ctxs[:n]).numpy()
        assert hn.shape == (n, 64)
        np.testing.assert_allclose(hn, h[:n], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(cn, c[:n], rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------- the seeding kernel as launched
@pytest.mark.parametrize("fmt", ["split", "f32"])
@pytest.mark.parametrize("H", [32, 512])
@pytest.mark.parametrize("B,beam", [(3, 3), (5, 1)])
def test_seed_context_kernel(B, beam, H, fmt):
    """through the ctypes table: the gathered rows bit-equal to their sources, ctx_prev / ctx_word at s * beam, nothing else written"""
    lib = _lib.lib()
    rng = np.random.RandomState(B * 1000 + beam * 100 + H)
    n_src, F = 7, 2
    G = F * B * beam
    if fmt == "split":      # split rows: pairs of f16, any bit pattern (the kernel copies records, it does not read values)
        src_h = rng.randint(-2 ** 31, 2 ** 31 - 1, size=(n_src, H), dtype=np.int64).astype(np.int32)
    else:
        src_h = rng.standard_normal((n_src, H)).astype(np.float32).view(np.int32)
    src_c = rng.standard_normal((n_src, H)).astype(np.float32).view(np.int32)
    last = rng.randint(0, 500, size=n_src).astype(np.int32)
    has = np.array([1, 0, 1, 1, 0, 1, 1], dtype=np.int32)
    idx = rng.randint(0, n_src, size=B).astype(np.int32)
    idx[0], idx[1] = 1, 6                                # a history of <eos> alone, and the last source row
    dst_h0 = rng.randint(-2 ** 31, 2 ** 31 - 1, size=(G + B, H), dtype=np.int64).astype(np.int32)
    dst_c0 = rng.randint(-2 ** 31, 2 ** 31 - 1, size=(G + B, H), dtype=np.int64).astype(np.int32)
    g = lambda a: torch.from_numpy(a.copy()).cuda()
    t = dict(src_h=g(src_h), src_c=g(src_c), last=g(last), has=g(has), idx=g(idx), dst_h=g(dst_h0), dst_c=g(dst_c0),
             prev=torch.full((B * beam,), -7, dtype=torch.int32, device="cuda"), word=torch.full((B * beam,), -9, dtype=torch.int32, device="cuda"))
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.jlm_seed_context(t["src_h"].data_ptr(), t["src_c"].data_ptr(), H, t["last"].data_ptr(), t["has"].data_ptr(), n_src,
                              t["idx"].data_ptr(), B, beam, G, t["dst_h"].data_ptr(), t["dst_c"].data_ptr(), t["prev"].data_ptr(),
                              t["word"].data_ptr(), st)
    assert rc == 0
    torch.cuda.synchronize()
    dh, dc = t["dst_h"].cpu().numpy(), t["dst_c"].cpu().numpy()
    prev, word = t["prev"].cpu().numpy(), t["word"].cpu().numpy()
    want_h, want_c = dst_h0.copy(), dst_c0.copy()
    want_prev, want_word = np.full(B * beam, -7, dtype=np.int32), np.full(B * beam, -9, dtype=np.int32)
    for s in range(B):
        r = int(idx[s])
        if has[r]:
            want_h[G + s], want_c[G + s] = src_h[r], src_c[r]
        want_prev[s * beam] = G + s if has[r] else -1
        want_word[s * beam] = last[r]
    assert np.array_equal(dh, want_h) and np.array_equal(dc, want_c)
    assert np.array_equal(prev, want_prev) and np.array_equal(word, want_word)
    # arguments the launcher refuses: nothing is launched
    bad = lambda **kw: lib.jlm_seed_context(t["src_h"].data_ptr(), t["src_c"].data_ptr(), kw.get("H", H), t["last"].data_ptr(),
                                            t["has"].data_ptr(), n_src, t["idx"].data_ptr(), B, kw.get("beam", beam), kw.get("G", G),
                                            t["dst_h"].data_ptr(), t["dst_c"].data_ptr(), t["prev"].data_ptr(), t["word"].data_ptr(), st)
    assert bad(H=6) == -1 and bad(beam=0) == -1 and bad(G=-1) == -1 and bad(G=2 ** 33) == -1


# ---------------------------------------------------------------------------------------------- the eval harness
EVAL_ARGV = ["-e", "1", "-es", "12", "-b", "10"]


def _run_eval(argv):
    from jlm_amd import eval as jeval
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        best, nbest = jeval.main(argv)
    return best, nbest, buf.getvalue()


def _body(name):
    with open(os.path.join("eval", name), "r", encoding="utf-8") as fh:
        body = fh.read()
    return body[:body.index("--- ")]                # (what follows are the run's timings)


@pytest.mark.parametrize("batch", [1, 16])
def test_eval_context_words(fx, batch, monkeypatch, tmp_path):
    from tests import golden_cases as gc
    f = fx("small-tied")
    lines = synth.write_test_corpus(f["root"], f["lexicon"], f["cfg"]["vocab_size"], **gc.EVAL_CORPUS)
    jconfig.set_root(f["root"])
    monkeypatch.chdir(tmp_path)
    argv = EVAL_ARGV + ["--batch", str(batch)]
    _run_eval(argv)
    names = sorted(os.listdir("eval"))
    assert len(names) == 1
    plain = _body(names[0])
    os.rename(os.path.join("eval", names[0]), "plain.txt")
    _run_eval(argv + ["--context_words", "0"])
    assert sorted(os.listdir("eval")) == names and _body(names[0]) == plain          # the same file name, the same bytes
    best, nbest, out = _run_eval(argv + ["-cw", "2"])
    assert names[0][:-len(".txt")] + "_ctx_2.txt" in os.listdir("eval")
    # the hit counts from primed-oracle decodes
    from jlm_amd.context import split_sentence
    from oracle import jlm_oracle as orc
    o = orc.OracleDecoder(f["root"], 1)
    surface = lambda t: t.split("/")[0]
    reading = lambda t: t.split("/")[1] if t.split("/")[1] != "" else t.split("/")[0]
    want_best = want_nbest = n = 0
    for line in lines:
        tokens = line.strip().split(" ")
        if any(o._check_oov(t) for t in tokens):
            continue
        ctx, rest = split_sentence(tokens, 2)
        assert len(ctx) == 2 and len(rest) == len(tokens) - 2
        x, y = "".join(reading(t) for t in rest), "".join(surface(t) for t in rest)
        sentences = ["".join(surface(w) for w in words) for _s, words in cc.primed_decode(o, x, [o.w2i[t] for t in ctx], beam_width=10)]
        want_best += y == sentences[0]
        want_nbest += y != sentences[0] and y in sentences
        n += 1
        if n >= 12:
            break
    assert (best, nbest) == (want_best, want_nbest)
    assert "best_hit {} nbest_hit{} ".format(want_best, want_nbest) in out
