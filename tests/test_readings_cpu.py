"""CPU-only: the reading index (jlm_amd/readings.py) and the host side of prediction from a typed reading prefix (jlm_amd/complete.py:
word sets, the numpy restatement of the masked row selection, the merge over padded lists, the argument checks and the CLI flags)."""
import numpy as np
import pytest

from jlm_amd import _lib, complete as C, ops as _ops, synth
from jlm_amd.data import CharVocab, Vocab
from jlm_amd.readings import ReadingIndex, reading_of, to_katakana

KANA = synth.KANA[:12]


@pytest.fixture(scope="module")
def small():
    lexicon, _rd = synth.make_lexicon(2000, alphabet=12)
    vocab = Vocab(2000, lexicon)
    return vocab, ReadingIndex(vocab)


def _brute(vocab, prefix, exact=False):
    out = []
    for i, (word, _f) in enumerate(vocab.lexicon):
        r = reading_of(word)
        if r is not None and (r == prefix if exact else r.startswith(prefix)):
            out.append(i)
    return out


def test_words_with_a_reading(small):
    vocab, index = small
    assert len(index) == 1998 and index.V == 2000
    assert reading_of("<unk>") is None and reading_of("<eos>") is None
    assert reading_of("w1/カキ/N") == "カキ" and reading_of("かき//N") == "かき"         # an empty token 1: token 0 (reading_dict's rule)
    everything = index.lookup("")
    assert len(everything) == 1998 and everything.dtype == np.int64
    assert vocab.w2i["<unk>"] not in everything and vocab.w2i["<eos>"] not in everything


def test_lookup_equals_a_scan(small):
    vocab, index = small
    sizes = {1: [], 2: [], "exact": []}
    prefixes = KANA + [a + b for a in KANA for b in KANA]
    rng = np.random.RandomState(0)
    prefixes += ["".join(KANA[c] for c in rng.randint(0, 12, size=3)) for _ in range(60)]
    for p in prefixes:
        for exact in (False, True):
            got = index.lookup(p, exact=exact)
            assert got.dtype == np.int64 and got.tolist() == _brute(vocab, p, exact), (p, exact)
            assert np.all(np.diff(got) > 0)
        if len(p) <= 2:
            sizes[len(p)].append(len(index.lookup(p)))
        if len(p) == 1:
            sizes["exact"].append(len(index.lookup(p, exact=True)))
    assert (min(sizes[1]), max(sizes[1])) == (140, 193)
    assert (min(sizes[2]), max(sizes[2])) == (6, 20)
    assert (min(sizes["exact"]), max(sizes["exact"])) == (4, 15)
    assert len(index.lookup(synth.KANA[40])) == 0               # a kana outside the 12-kana alphabet


def test_unused_prefixes_at_50000_words():
    lexicon, _rd = synth.make_lexicon(50000)
    index = ReadingIndex(Vocab(50000, lexicon))
    empty = [a + b for a in synth.KANA for b in synth.KANA if len(index.lookup(a + b)) == 0]
    assert len(empty) == 4
    got = index.lookup(empty[0])
    assert got.dtype == np.int64 and got.shape == (0,)


def test_hiragana_is_folded(small):
    _vocab, index = small
    assert to_katakana("きょう") == "キョウ" and to_katakana("キョa") == "キョa"
    for p in (KANA[3], KANA[3] + KANA[7], KANA[11] + KANA[0]):
        hira = "".join(chr(ord(c) - 0x60) for c in p)
        assert hira != p and to_katakana(hira) == p
        assert np.array_equal(index.lookup(hira), index.lookup(p)) and len(index.lookup(p))
        assert np.array_equal(index.lookup(hira, exact=True), index.lookup(p, exact=True))


def test_char_vocab_is_refused():
    lexicon, _rd = synth.make_lexicon(300, alphabet=12, display_alphabet=50)
    with pytest.raises(ValueError):
        ReadingIndex(CharVocab(300, lexicon))


def test_mask_bits(small):
    _vocab, index = small
    V = 2000
    lists = [index.lookup(KANA[0]), index.lookup(KANA[1] + KANA[2]), np.array([], dtype=np.int64), index.lookup(KANA[0])[::-1],
             np.array([0, 31, 32, 1999, 1999])]
    mask, which = ReadingIndex.mask(lists, V)
    assert mask.dtype == np.uint32 and mask.shape == (4, 63) and which.tolist() == [0, 1, 2, 0, 3]       # equal lists share a set
    for ids, s in zip(lists, which):
        bits = [w for w in range(mask.shape[1] * 32) if (int(mask[s, w >> 5]) >> (w & 31)) & 1]
        assert bits == sorted(set(np.asarray(ids).tolist()))
        assert all(w < V for w in bits)                                                                # nothing at or beyond V
    mask, which = ReadingIndex.mask([], 70)
    assert mask.shape == (0, 3) and len(which) == 0
    assert ReadingIndex.mask([[69]], 70)[0][0].tolist() == [0, 0, 32]
    for bad in ([70], [-1]):
        with pytest.raises(ValueError):
            ReadingIndex.mask([bad], 70)


def _direct(y, k, allowed, self_norm):
    yd = np.asarray(y, dtype=np.float32).astype(np.float64)
    cand = sorted((w for w in set(allowed) if not np.isnan(yd[w])), key=lambda w: (-yd[w], w))[:k]
    m = yd.max()
    lse = m + np.log(np.exp(yd - m).sum())
    nll = [(-yd[w] if self_norm else lse - yd[w]) for w in cand]
    return cand + [-1] * (k - len(cand)), nll + [np.inf] * (k - len(cand))


def test_topk_masked_reference_against_a_direct_sort():
    rng = np.random.RandomState(1)
    for trial in range(40):
        n = int(rng.randint(1, 60))
        y = rng.randint(-3, 4, size=n).astype(np.float32) * 0.5            # ties everywhere
        k = int(rng.randint(1, n + 1))
        allowed = np.flatnonzero(rng.rand(n) < rng.rand())
        for sn in (False, True):
            ids, nll = C.topk_masked_reference(y, k, allowed, sn)
            want_ids, want_nll = _direct(y, k, allowed.tolist(), sn)
            assert ids.dtype == np.int64 and nll.dtype == np.float64 and ids.tolist() == want_ids
            np.testing.assert_allclose(nll, want_nll, rtol=0, atol=1e-12)
    y = np.array([0.5, 3.0, -1.0, 3.0, 9.0, 2.0], dtype=np.float32)
    ids, nll = C.topk_masked_reference(y, 4, [5, 3, 1, 3])                  # the maximum (word 4) is not allowed; 3 words, k = 4
    assert ids.tolist() == [1, 3, 5, -1] and nll[3] == np.inf
    lse = np.log(np.exp(y.astype(np.float64)).sum())                      # ... and the normaliser still counts it
    np.testing.assert_allclose(nll[:3], lse - np.array([3.0, 3.0, 2.0]), rtol=0, atol=1e-12)
    assert C.topk_masked_reference(y, 2, [])[0].tolist() == [-1, -1]
    full = C.topk_masked_reference(y, 6, np.arange(6))                      # every word allowed: the unmasked restatement
    assert full[0].tolist() == C.topk_reference(y, 6)[0].tolist() and np.array_equal(full[1], C.topk_reference(y, 6)[1])
    y[2] = -np.inf
    y[0] = np.nan                                                         # -inf ranks (last), NaN never does
    assert C.topk_masked_reference(y, 3, [0, 2, 5], self_norm=True)[0].tolist() == [5, 2, -1]


def test_merge_reference_on_padded_first_frame_lists():
    B = 4
    y = np.array([[0.0, 1.0, 2.0, 3.0, 4.0, 5.0], [5.0, 4.0, 3.0, 2.0, 1.0, 0.0]], dtype=np.float32)
    lists = [C.topk_masked_reference(y[0], B, [1, 4]), C.topk_masked_reference(y[1], B, [])]
    ci = np.array([l[0] for l in lists], dtype=np.int32)
    cn = np.array([l[1] for l in lists])
    out = C.merge_reference(ci, cn, None, None, B, 2, first=True, stop_id=-1)
    assert out["bp_word"].tolist() == [4, 1, -1, -1] + [-1] * 4
    assert out["finished"].tolist() == [0, 0, 1, 1] + [1] * 4               # a padded candidate is a finished hypothesis ...
    assert np.isfinite(out["score"][:2]).all() and np.isinf(out["score"][2:]).all()       # ... of infinite score
    assert out["word"].tolist() == [4, 1, 0, 0] + [0] * 4                   # that steps a valid word
    assert out["prev"].tolist() == [0] * 4 + [1] * 4
    # the next frame: the two live parents offer a full beam, the carries of the padding drop out
    nxt = [C.topk_reference(y[0], B), C.topk_reference(y[1], B)] + [C.topk_reference(y[0], B)] * 2
    ci2 = np.array([l[0] for l in nxt], dtype=np.int32)
    cn2 = np.array([l[1] for l in nxt])
    out2 = C.merge_reference(ci2, cn2, out["score"][:4], out["finished"][:4], B, 1, first=False, stop_id=-1)
    assert np.isfinite(out2["score"]).all() and set(out2["bp_parent"].tolist()) <= {0, 1} and (out2["bp_word"] >= 0).all()
    # with one live parent and B = 4 the parent's four candidates fill the beam; with a finished live parent the carries stay
    fin = np.array([1, 1, 1, 1], dtype=np.int32)
    out3 = C.merge_reference(ci2, cn2, out["score"][:4], fin, B, 1, first=False, stop_id=-1)
    assert out3["bp_word"].tolist() == [-1] * 4 and out3["bp_parent"].tolist() == [0, 1, 2, 3]
    assert np.isinf(out3["score"][2:]).all() and out3["finished"].tolist() == [1] * 4


class _NoDevice:
    """a backend and a completer that fail the test when anything reaches them"""

    class m:
        V, H, ldt = 100, 8, 8

    def __getattr__(self, name):
        raise AssertionError("reached the backend: " + name)

    def row_bytes(self, *a):
        return 1024

    def run(self, *a, **kw):
        raise AssertionError("reached the device")


def test_word_set_arguments_are_checked_before_any_launch(monkeypatch):
    monkeypatch.setattr(_ops, "_backend", _NoDevice())
    comp = _NoDevice()
    comp.m = _NoDevice.m
    bad = [[[100]], [[-1]], [[1.5]], [[[1, 2]]], [[1], [2]], []]
    for allowed in bad:
        with pytest.raises(ValueError):
            C.predict_top(comp, [[1, 2]], n=5, allowed=allowed)
        with pytest.raises(ValueError):
            C.complete(comp, [[1, 2]], 3, beam_width=5, first_allowed=allowed)
    assert C.check_allowed(None, 3, 100, "x") is None
    sets = C.check_allowed([None, [7, 3, 7], np.array([], dtype=np.int64)], 3, 100, "x")
    assert sets[0] is None and sets[1].tolist() == [3, 7] and sets[1].dtype == np.int64 and sets[2].tolist() == []
    # an empty set: empty results, and nothing reaches the device
    res = C.predict_top(comp, [[1, 2], [3]], n=5, allowed=[[], np.array([], dtype=np.int64)])
    assert [(r[0].tolist(), r[1].tolist()) for r in res] == [([], []), ([], [])]
    assert res[0][0].dtype == np.int64 and res[0][1].dtype == np.float64
    assert C.complete(comp, [[1, 2]], 3, beam_width=5, first_allowed=[[]]) == [[]]
    with pytest.raises(AssertionError):                                     # (a set with a word does reach it)
        C.complete(comp, [[1, 2]], 3, beam_width=5, first_allowed=[[4]])


def test_cli_flags_and_entry_points():
    ap = C.build_parser()
    a = ap.parse_args(["--prompt", "w1/カ/N", "--top", "5", "--reading", "きょ", "--exact"])
    assert a.reading == "きょ" and a.exact and a.top == 5
    a = ap.parse_args(["--words", "4", "--reading", "キ"])
    assert a.reading == "キ" and not a.exact and a.top is None and a.words == 4
    a = ap.parse_args([])
    assert a.reading is None and not a.exact
    with pytest.raises(SystemExit):
        C.main(["--exact"])                                                 # --exact needs --reading: refused before anything loads
    for n in ("jlm_topk_rows_masked", "jlm_complete_frames_masked"):
        assert n in _lib.EXPORTS
