"""CPU-only: the host logic of teacher-forced scoring (jlm_amd/score.py, jlm_amd/perplexity.py) -- corpus encoding as the reference's
Corpus.encode_corpus does it, the corpus_iterator stream layout, the row plan of a sentence-mode call, and the id checks that run
before any launch.  The device side is covered by tests/test_gpu_score.py."""
import numpy as np
import pytest

from jlm_amd import config as jconfig, synth
from jlm_amd.data import CharVocab, Vocab
from jlm_amd.perplexity import encode_lines, read_lines
from jlm_amd.rowsets import check_ids
from jlm_amd.score import plan_rows, sentence_arrays, stream_layout


def test_encoding_falls_back_to_unk_and_ends_lines_with_eos(fx):
    f = fx("small-vtable")
    V = f["cfg"]["vocab_size"]
    lines = synth.write_test_corpus(f["root"], f["lexicon"], V, 12, words_per_sentence=5, seed=11, oov_every=3)
    jconfig.set_root(f["root"])
    vocab = Vocab(V)
    got, n_unk = encode_lines(read_lines(jconfig.data_path + "/test.txt"), vocab)
    assert len(got) == len(lines) == 12
    eos, unk = vocab.w2i["<eos>"], vocab.w2i["<unk>"]
    for line, ids in zip(lines, got):
        words = line.split(" ")
        assert len(ids) == len(words) + 1 and ids[-1] == eos
        assert ids[:-1] == [vocab.w2i.get(w, unk) for w in words]
    assert n_unk == 4 and sum(ids.count(unk) for ids in got) == 4        # one out-of-vocabulary word in every third line
    head, _ = encode_lines(read_lines(jconfig.data_path + "/test.txt", 5), vocab)
    assert head == got[:5]


def test_char_vocab_encoding(fx):
    f = fx("small-char")
    jconfig.set_root(f["root"])
    vocab = CharVocab(f["cfg"]["vocab_size"])
    surf = [w.split("/")[0] for w, _ in f["lexicon"][2:6]]
    lines = [" ".join(f["lexicon"][i][0] for i in range(2, 6)), "☃ " + f["lexicon"][3][0], ""]
    got, n_unk = encode_lines(lines, vocab)
    c2i = vocab.c2i
    assert got[0] == [c2i[c] for c in "".join(surf)] + [c2i["<eos>"]]
    assert got[1] == [c2i["<unk>"]] + [c2i[c] for c in surf[1]] + [c2i["<eos>"]]
    assert got[2] == [c2i["<eos>"]]                    # an empty line: no characters, the <eos>
    assert n_unk == 1


def _corpus_iterator(raw, batch_size, num_steps):
    """train/utils.py:17-31 restated: rows of batch_len = len // batch_size, epoch_size = (batch_len - 1) // num_steps chunks"""
    batch_len = len(raw) // batch_size
    data = [raw[batch_len * i:batch_len * (i + 1)] for i in range(batch_size)]
    epoch_size = (batch_len - 1) // num_steps
    if epoch_size == 0:
        raise ValueError("epoch_size == 0")
    for i in range(epoch_size):
        yield ([d[i * num_steps:(i + 1) * num_steps] for d in data], [d[i * num_steps + 1:(i + 1) * num_steps + 1] for d in data])


@pytest.mark.parametrize("n,batch_size,num_steps", [(1000, 7, 5), (1000, 10, 20), (97, 4, 3), (41, 4, 9)])
def test_stream_layout_is_corpus_iterator(n, batch_size, num_steps):
    raw = list(np.random.RandomState(n).randint(0, 500, size=n))
    x, y = stream_layout(raw, batch_size, num_steps)
    chunks = list(_corpus_iterator(raw, batch_size, num_steps))
    assert x.shape == y.shape == (batch_size, len(chunks) * num_steps) and x.dtype == np.int32
    for i, (cx, cy) in enumerate(chunks):
        np.testing.assert_array_equal(x[:, i * num_steps:(i + 1) * num_steps], np.array(cx))
        np.testing.assert_array_equal(y[:, i * num_steps:(i + 1) * num_steps], np.array(cy))
    np.testing.assert_array_equal(x[:, 1:], y[:, :-1])      # targets are the inputs shifted by one
    assert x.size < n                                       # the tail is dropped


def test_stream_layout_too_short():
    with pytest.raises(ValueError):
        stream_layout(list(range(30)), 8, 5)


def test_row_plan():
    rng = np.random.RandomState(3)
    lens = list(rng.randint(0, 41, size=700)) + [0, 0, 40]
    chunks = plan_rows(lens, 256)
    seen = np.concatenate([c["idx"] for c in chunks])
    nonempty = [i for i, L in enumerate(lens) if L > 0]
    assert sorted(seen.tolist()) == nonempty                # every non-empty sequence once, empty ones take no row
    assert all(len(c["idx"]) <= 256 for c in chunks) and len(chunks) == (len(nonempty) + 255) // 256
    flat = [lens[i] for i in seen]
    assert flat == sorted(flat, reverse=True)               # longest first ...
    for i in range(1, len(seen)):                           # ... stable among equals
        if flat[i] == flat[i - 1]:
            assert seen[i] > seen[i - 1]
    for c in chunks:
        L = np.array([lens[i] for i in c["idx"]])
        assert c["n_steps"] == L.max() and len(c["n_live"]) == c["n_steps"]
        for t, k in enumerate(c["n_live"]):
            assert k == (L > t).sum() and (L[:k] > t).all()      # the live rows of step t are a prefix
    inv = np.empty(len(lens), dtype=np.int64)
    inv[:] = -1
    inv[seen] = np.arange(len(seen))
    assert all(inv[i] >= 0 for i in nonempty) and all(seen[inv[i]] == i for i in nonempty)
    assert plan_rows([0, 0], 8) == [] and plan_rows([], 8) == []
    with pytest.raises(ValueError):
        plan_rows([1], 0)


def test_sentence_arrays():
    word, target = sentence_arrays([[5, 6, 7], [8]], 1, 3)
    np.testing.assert_array_equal(word, [[1, 1], [5, 0], [6, 0]])
    np.testing.assert_array_equal(target, [[5, 8], [6, 0], [7, 0]])


def test_bad_ids_raise_before_any_launch(fx, monkeypatch):
    check_ids([0, 1, 1999], 2000, "x")
    for bad in ([2000], [-1], [[3, 4], [5, 2001]]):
        with pytest.raises(ValueError, match="outside"):
            check_ids(bad, 2000, "x")
    # through the public API: the model's scorer rejects the ids before it touches the device
    from jlm_amd import score as jscore

    class _Dev:
        V, H = 2000, 8

    class _NoLaunch(jscore.Scorer):
        def __init__(self):
            self.m = _Dev()

        def run(self, *a, **k):
            raise AssertionError("launched")

        def row_bytes(self, n_steps, per_token=True):
            return 1 << 20

    for seqs, start in (([[1, 2], [3, 2000]], 1), ([[1, 2]], -3), ([[1], [-1, 4]], 1)):
        with pytest.raises(ValueError):
            jscore.score_sequences(_NoLaunch(), seqs, start)
