"""CPU: per-segment candidate lists behind a decode (Decoder.decode_candidates) -- the yardstick
(tests/candidate_cases.py) against the conditions the GPU bars rest on, the host path end to end over the numpy double of the new op
(tests/fake_alt.py), every refusal, and that a failure in phase 2 leaves no plan busy."""
import numpy as np
import pytest

from tests import candidate_cases as kc
from tests import context_cases as cc
from tests import fake_alt


@pytest.fixture()
def fake(monkeypatch):
    return fake_alt.install(monkeypatch)


def _decoder(name):
    cc.set_root(name)
    from jlm_amd.decoder import Decoder
    d = Decoder(1)
    d.perf_timing = False
    return d


# ---------------------------------------------------------------------------------------------- the yardstick checks itself
@pytest.mark.parametrize("with_ctx", [False, True], ids=["plain", "context"])
@pytest.mark.parametrize("name", list(cc.MODELS))
def test_yardstick_conditions(name, with_ctx):
    """what the GPU bars rest on: the own word's total is the 1-best score to 1e-9; with lookahead=None every adjacent pair inside a
    segment's first 11 entries is more than 1e-4 apart (no position is exempt); at beam 1 some alternative scores below the path"""
    n_alt = 0
    for beam in cc.BEAMS:
        better = 0
        for (conv, own, segs), (_c, lists) in zip(kc.path_terms(name, beam, with_ctx), kc.yardstick(name, beam, with_ctx)):
            if own is None:
                continue
            assert abs(own.sum() - conv[0][0]) <= 1e-9, (name, beam, conv[0])
            for k, ((_s, _l, alts), (_s2, _l2, cands)) in enumerate(zip(segs, lists)):
                mine = [kc.totals(own, t, k, None) for w, t in alts if w == conv[0][1][k]]
                assert mine and min(abs(x - conv[0][0]) for x in mine) <= 1e-9, (name, beam, k)
                sc = [x for x, _w in cands]
                assert all(b - a > kc.SEPARATION for a, b in zip(sc, sc[1:])), (name, beam, with_ctx, k, sc)
                assert all(kc.separated(cands)), (name, beam, with_ctx, k)
                better += sum(1 for w, t in alts if kc.totals(own, t, k, None) < conv[0][0] - 1e-9)
                n_alt += len(alts)
        if beam == 1:
            assert better >= 1, (name, with_ctx)
    assert n_alt >= 150


@pytest.mark.parametrize("name", list(cc.MODELS))
def test_yardstick_separation_at_finite_lookaheads(name):
    """lookahead 0 and 1: the same separation, but for at most MAX_EXEMPT positions per (model, beam) -- the union over contexts,
    lookaheads and ranks -- and they are the ones candidate_cases.EXPECTED_CLOSE names: with contexts, at lookahead 0"""
    expected = kc.EXPECTED_CLOSE.get(name, set())
    assert len(expected) <= kc.MAX_EXEMPT
    for beam in cc.BEAMS:
        union = set()
        for with_ctx in (False, True):
            for la in kc.LOOKAHEADS:
                for rank in (0, 1):
                    close = set(kc.close_positions(name, with_ctx, beam, la, rank))
                    assert not close or (with_ctx and la == 0), (name, with_ctx, beam, la, rank, close)
                    union |= close
        assert len(union) <= kc.MAX_EXEMPT and union <= expected, (name, beam, sorted(union))
    assert not expected or any(kc.close_positions(name, True, beam, 0, 0) for beam in cc.BEAMS), name


# ---------------------------------------------------------------------------------------------- the host path over the double
@pytest.mark.parametrize("with_ctx", [False, True], ids=["plain", "context"])
@pytest.mark.parametrize("name", list(cc.MODELS))
def test_host_path_end_to_end(name, with_ctx, fake):
    dec = _decoder(name)
    texts = kc.inputs()
    ctxs = kc.contexts(cc.MODELS[name][0]) if with_ctx else None
    for beam in cc.BEAMS:
        conv = dec.decode_batch(texts, topN=kc.TOPN, beam_width=beam, context=ctxs)
        exempt = set()                                       # per (model, beam), over the lookaheads and ranks
        for la in kc.LOOKAHEADS:
            for rank in (0, 1):
                got = dec.decode_candidates_batch(texts, topN=kc.TOPN, beam_width=beam, n_cand=kc.N_CAND, lookahead=la, rank=rank,
                                                  context=ctxs)
                assert len(got) == len(texts)
                want = kc.yardstick(name, beam, with_ctx, la, rank)
                for i, ((c, segs), (yc, lists)) in enumerate(zip(got, want)):
                    assert c == conv[i], (name, beam, i)
                    if len(yc) <= rank or not texts[i]:
                        assert segs == [], (name, beam, la, rank, i)
                        continue
                    close = {(i, k, pos) for k, pos in kc.check_segments(segs, lists, c, rank, (name, beam, la, rank, i))}
                    assert la == 0 or not close, (name, beam, la, rank, close)
                    exempt |= close
                assert got[-1] == ([(0.0, [])], [])
        assert len(exempt) <= kc.MAX_EXEMPT and exempt <= kc.EXPECTED_CLOSE.get(name, set()), (name, beam, exempt)
    assert not any(p.busy for p in dec._engine.plans)


def test_batch_shape_does_not_matter(fake):
    """one input, the batch in three chunks, another order, a row budget that splits a segment's alternatives over two device calls"""
    dec = _decoder("tied")
    texts = kc.inputs()
    got = dec.decode_candidates_batch(texts, beam_width=5)
    one = dec.decode_candidates(texts[4], topN=3, beam_width=5, n_cand=4)
    assert one[0] == dec.decode(texts[4], topN=3, beam_width=5)
    assert one[1] == [(s, ln, c[:4]) for s, ln, c in got[4][1]]
    assert {n.word for n in dec.backward_lookup[len(texts[4])]}
    dec.max_batch = 5
    assert dec.decode_candidates_batch(texts, beam_width=5) == got
    dec.max_batch = 1024
    perm = list(reversed(range(len(texts))))
    assert dec.decode_candidates_batch([texts[i] for i in perm], beam_width=5) == [got[i] for i in perm]
    n_alts = max(len(c) for _conv, segs in dec.decode_candidates_batch(texts, beam_width=5, n_cand=64) for _s, _l, c in segs)
    assert n_alts >= 3
    dec._engine.ALT_MAX_ROWS = n_alts - 1                      # some segment's alternatives fall into two calls
    fake.launches.clear()
    assert dec.decode_candidates_batch(texts, beam_width=5) == got
    assert fake.launches.count("alt_head") >= 2
    dec._engine.ALT_MAX_ROWS = None
    assert dec.decode_candidates_batch([], beam_width=5) == []
    assert dec.decode_candidates("", beam_width=5) == ([(0.0, [])], [])
    assert dec.decode_candidates_batch(["", ""], beam_width=5) == [([(0.0, [])], [])] * 2


def test_lookahead_zero_runs_the_head_launch_only(fake):
    dec = _decoder("tied")
    texts = kc.inputs()
    fake.launches.clear()
    dec.decode_candidates_batch(texts, beam_width=5, lookahead=0)
    assert fake.launches == ["alt_head"]
    fake.launches.clear()
    dec.decode_candidates_batch(texts, beam_width=5, lookahead=2)
    assert fake.launches == ["alt_head", "score_step", "score_step"]


def test_plans_of_plain_decodes_are_untouched(fake):
    """phase 2 borrows the decode's own plan: no new plan flavour, no new key"""
    dec = _decoder("tied")
    texts = kc.inputs()[:4]
    dec.decode_batch(texts, beam_width=5)
    keys = {p.key for p in dec._engine.plans}
    dec.decode_candidates_batch(texts, beam_width=5)
    assert {p.key for p in dec._engine.plans} == keys


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch(fake, monkeypatch):
    dec = _decoder("tied")
    texts = kc.inputs()[:3]
    launched = []
    monkeypatch.setattr(dec._engine, "submit", lambda *a, **k: launched.append(1))
    monkeypatch.setattr(dec.model, "prime", lambda *a, **k: launched.append(2))
    with pytest.raises(ValueError):
        dec.decode_candidates_batch(texts, beam_width=None)
    with pytest.raises(ValueError):
        dec.decode_candidates_batch(texts, beam_width=0)
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError):
            dec.decode_candidates_batch(texts, n_cand=bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            dec.decode_candidates_batch(texts, lookahead=bad)
    for bad in (-1, 10, 0.5):
        with pytest.raises(ValueError):
            dec.decode_candidates_batch(texts, topN=10, rank=bad)
    with pytest.raises(ValueError):
        dec.decode_candidates_batch(texts, topN=1, rank=1)
    dec.compat_quirks, dec.lattice_vocab = True, [1, 2, 3]
    with pytest.raises(ValueError):
        dec.decode_candidates(texts[0])
    dec.compat_quirks, dec.lattice_vocab = False, None
    dec.CAND_LIMIT = 1                                       # every cell is too large for the device beam step
    with pytest.raises(ValueError) as e:
        dec.decode_candidates_batch(texts, beam_width=5, context=[[5], [6], [7]])
    assert repr(texts[0]) in str(e.value) and "0 (" in str(e.value)
    dec.CAND_LIMIT = None
    for kw in (dict(vocab_select=True), dict(cache=None), dict(ngram=None)):
        with pytest.raises(TypeError):
            dec.decode_candidates_batch(texts, **kw)         # there are no such arguments
    assert not launched


def test_a_cached_context_is_refused(fake):
    from jlm_amd.cache import CacheSpec
    from jlm_amd.context import CachedContext
    dec = _decoder("tied")
    z = np.zeros(1, dtype=np.int32)
    state = CachedContext(dec.model.dev, None, None, None, None, z, z, None, np.zeros((1, 1), dtype=np.int32), None, z,
                          CacheSpec(theta=0.3, lam=0.0, size=8))
    with pytest.raises(ValueError):
        dec.decode_candidates_batch(kc.inputs()[:1], context=state)
    state.spec = CacheSpec(theta=0.3, lam=0.2, size=8)
    with pytest.raises(ValueError):
        dec.decode_candidates_batch(kc.inputs()[:1], context=state)


def test_other_decoders_raise_type_error(fake):
    cc.set_root("tied")
    from jlm_amd.decoder_dynamic import DynamicDecoder
    from jlm_amd.decoder_char import CharRNNDecoder
    from jlm_amd.decoder_ngram import NGramDecoder
    d = DynamicDecoder(1)
    with pytest.raises(TypeError):
        d.decode_candidates("アイ")
    with pytest.raises(TypeError):
        d.decode_candidates_batch(["アイ"])
    for cls in (CharRNNDecoder, NGramDecoder):
        obj = cls.__new__(cls)                               # (the refusal needs no model)
        with pytest.raises(TypeError):
            obj.decode_candidates("アイ")
        with pytest.raises(TypeError):
            obj.decode_candidates_batch(["アイ"])


def test_a_failure_in_phase_two_leaves_no_plan_busy(fake):
    dec = _decoder("tied")
    texts = kc.inputs()
    dec.max_batch = 5
    fake.fail_alt = RuntimeError("phase 2")
    with pytest.raises(RuntimeError, match="phase 2"):
        dec.decode_candidates_batch(texts, beam_width=5)
    assert dec._engine.plans and not any(p.busy for p in dec._engine.plans)
    fake.fail_alt = None
    dec.max_batch = 1024
    want = dec.decode_batch(texts, beam_width=5)
    assert [c for c, _s in dec.decode_candidates_batch(texts, beam_width=5)] == want


def test_engine_refuses_a_released_plan(fake):
    dec = _decoder("tied")
    from jlm_amd.lattice import BatchLattice
    lat = BatchLattice(dec._builder, kc.inputs()[:2], 3)
    ticket = dec._engine.submit(lat, "static")
    dec._engine.collect(ticket)
    with pytest.raises(ValueError):
        dec._engine.candidates(ticket)


def test_the_double_refuses_what_the_launcher_refuses(fake):
    """the launcher's refusals, restated: -1 without a launch"""
    from jlm_amd import _lib
    seg = (_lib.Segment * 1)(_lib.Segment(0, 8, 8, 0, 64, 8))
    buf = np.zeros(256, dtype=np.float64)
    ptr = buf.ctypes.data + (-buf.ctypes.data) % 16              # (the refusals look at the pointers, never through them)

    def plans(**kw):
        a, p = _lib.AltPlan(), _lib.ScorePlan()
        a.n_sent, a.beam, a.n_frames, a.rank = 1, 2, 3, 0
        for f in ("h", "c", "T", "score", "lse", "bp", "sent_len", "sent_off", "sent_rows", "depth", "alt", "prev0"):
            setattr(a, f, ptr)
        p.n_rows, p.n_steps = 2, 0
        p.h[0], p.c[0], p.prev0, p.nll_seq = ptr, ptr, ptr, ptr
        for k, v in kw.items():
            setattr(a if hasattr(a, k) else p, k, v)
        return a, p
    ok = plans()
    assert fake.jlm_alt_head_refuse(seg, 1, ptr, 8, 8, 0, *ok) == 0
    for kw in (dict(beam=0), dict(beam=1025), dict(rank=2), dict(rank=-1), dict(T=None), dict(T=ptr + 4), dict(h=ptr + 8), dict(lse=None),
               dict(score=ptr + 4), dict(bp=ptr + 2), dict(prev0=ptr + 4), dict(nll_seq=None), dict(n_frames=0)):
        assert fake.jlm_alt_head_refuse(seg, 1, ptr, 8, 8, 0, *plans(**kw)) == -1, kw
    assert fake.jlm_alt_head_refuse(seg, 1, ptr, 6, 8, 0, *ok) == -1             # ldt % 4
    assert fake.jlm_alt_head_refuse(seg, 1, ptr, 8, 6, 0, *ok) == -1             # H % 4
    assert fake.jlm_alt_head_refuse(seg, 1, ptr, 8, 8, 2, *ok) == -1             # mode
    assert fake.jlm_alt_head_refuse(seg, 1, ptr, 48 * 1024, 8, 0, *ok) == -1     # LDS
    assert fake.jlm_alt_head_refuse(seg, 1, ptr, 8, 8, 1, *plans(lse=None)) == 0  # mode 1 reads no lse
    assert not fake.launches


# ---------------------------------------------------------------------------------------------- eval harness and command line
def test_eval_candidates_counts_are_consistent(fx, fake, monkeypatch, tmp_path, capsys):
    import os
    from jlm_amd import config as jconfig, eval as jeval, synth
    from tests import golden_cases as gc
    f = fx("small-tied")
    synth.write_test_corpus(f["root"], f["lexicon"], f["cfg"]["vocab_size"], **gc.EVAL_CORPUS)
    jconfig.set_root(f["root"])
    monkeypatch.chdir(tmp_path)
    os.makedirs("eval", exist_ok=True)
    p = jeval.build_parser()
    assert not hasattr(p.parse_args([]), "candidates") and p.parse_args(["--candidates", "7"]).candidates == 7
    sents, wrong, le1, le5, len_, fixable = jeval.main(["-e", "1", "-es", "8", "-b", "2", "--batch", "4", "--candidates", "7"])
    assert 0 <= sents <= 8 and wrong >= sents and le1 <= le5 <= len_ <= wrong and fixable <= sents
    out = capsys.readouterr().out
    assert "candidates 7 same_seg_wrong %d wrong_segments %d " % (sents, wrong) in out and " eval_size 8" in out
    (name,) = os.listdir("eval")
    assert name.endswith("_cand_7.txt")
    with open(os.path.join("eval", name), encoding="utf-8") as fh:
        assert fh.read().count(" position ") == wrong
    for bad in (["-vs", "1"], ["-dd", "1"], ["-ng", "1"], ["--cut_last", "1"]):
        with pytest.raises(ValueError):
            jeval.Evaluator(p.parse_args(["-e", "1", "--candidates", "7"] + bad))
    with pytest.raises(ValueError):
        jeval.Evaluator(p.parse_args(["-e", "1", "--candidates", "65"]))
    # without the flag the harness's lines and log names are what they were
    jeval.main(["-e", "1", "-es", "8", "-b", "2", "--batch", "4"])
    assert sorted(n.endswith("_cand_7.txt") for n in os.listdir("eval")) == [False, True]
    assert "candidates" not in capsys.readouterr().out


def test_command_line_prints_the_segments(fake, capsys):
    from jlm_amd import complete
    text = kc.inputs()[4]
    cc.set_root("tied")
    res = complete.main(["--root", cc.model_root("tied"), "-e", "1", "--candidates", text, "-b", "5", "--n-cand", "4", "--lookahead", "1"])
    out = capsys.readouterr().out.splitlines()
    out = out[out.index("conversion:"):]                 # (the model's load line comes first)
    (conv, segs), = res
    assert out[1].split("\t")[0] == " ".join(w.split("/")[0] for w in conv[0][1])
    assert len(out) == 2 + len(segs) + sum(len(c) for _s, _l, c in segs) and all(len(c) <= 4 for _s, _l, c in segs)
    assert [ln for ln in out if ln.startswith("segment ")][0] == "segment %d+%d %s:" % (segs[0][0], segs[0][1], text[:segs[0][1]])
    dec_ref = _decoder("tied").decode_candidates(text, topN=1, beam_width=5, n_cand=4, lookahead=1)
    assert res[0] == dec_ref
    with pytest.raises(SystemExit):
        complete.main(["--root", cc.model_root("tied"), "-e", "1", "--candidates", text, "--convert", text])
