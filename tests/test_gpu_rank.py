"""GPU: LSTM_Model.rank / rank_streams end to end (jlm_amd/rank.py; csrc jlm_rank_frames + rank_rows_kernel) on the models of
tests/context_cases.py -- tied, V_table, D-softmax, untied at H = 64 and a tied model at H = 512, whose LSTM step runs other kernels.

The yardstick is tests/rank_cases.py: every device rank lies in the interval the oracle's float64 logits leave open at 1e-4 (no
exemptions; tests/test_rank_cpu.py asserts that the interval is a single rank for more than 80 % of the entries).  The ranks agree with
what the selection kernels return for the same history (predict_top, predict_reading), are the same bits however the rows are ordered
and cut into calls and whether the state is carried or not, and a ranking call leaves score() of the same model object as it was."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import context_cases as cc                                                     # noqa: E402
from tests import rank_cases as rc                                                        # noqa: E402

pytestmark = pytest.mark.gpu

_MODEL, _RANKS = {}, {}


def model(name):
    """the model, loaded once for the module"""
    if name not in _MODEL:
        cc.set_root(name)
        from jlm_amd.model import LSTM_Model
        _MODEL[name] = LSTM_Model(experiment_id=1)
    cc.set_root(name)
    return _MODEL[name]


def ranks(name):
    """rank() of the yardstick's sequences, computed once and left unchanged"""
    if name not in _RANKS:
        _RANKS[name] = model(name).rank(rc.sequences(cc.MODELS[name][0]), cc.EOS)
    return _RANKS[name]


@pytest.mark.parametrize("name", rc.GPU_MODELS)
def test_every_rank_inside_the_oracle_interval(name):
    got = ranks(name)
    seqs = rc.sequences(cc.MODELS[name][0])
    assert [g.shape for g in got] == [(len(s), rc.MAX_PREFIX + 3) for s in seqs]
    rc.check_in_bounds(got, name)


@pytest.mark.parametrize("name", rc.GPU_MODELS)
def test_column_a_agrees_with_predict_top(name):
    m, got = model(name), ranks(name)
    seqs = rc.sequences(cc.MODELS[name][0])
    contexts = [[cc.EOS] + s[:i] for s in seqs for i in range(len(s))]
    targets = [t for s in seqs for t in s]
    a = np.concatenate([g[:, 0] for g in got])
    for k in (1, 5, 10):
        top = m.predict_top(contexts, n=k)
        member = np.array([t in ids.tolist() for t, (ids, _lp) in zip(targets, top)])
        assert np.array_equal(a < k, member), (name, k, np.flatnonzero((a < k) != member)[:5].tolist())


@pytest.mark.parametrize("name", rc.GPU_MODELS)
def test_reading_levels_agree_with_predict_reading(name):
    """one row: after j typed kana the target is among predict_reading's k words exactly when its level-j rank is below k; the same
    for its homophones with exact=True"""
    m, got = model(name), ranks(name)
    index = m.reading_index()
    s, g = rc.sequences(cc.MODELS[name][0])[1], got[1]
    reading = {int(i): r for r, i in zip(index.readings, index.ids)}
    contexts, typed, col, tok = [], [], [], []
    for i, t in enumerate(s):
        if t in reading:
            for j in range(len(reading[t]) + 1):
                contexts.append([cc.EOS] + s[:i]); typed.append(reading[t][:j]); col.append(1 + j); tok.append(i)
    assert len(contexts) >= 20
    k = 5
    top = m.predict_reading(contexts, typed, n=k)
    for (ids, _lp), i, c in zip(top, tok, col):
        assert (g[i, c] < k) == (s[i] in ids.tolist()), (name, i, c, g[i], ids)
    words = [i for i, t in enumerate(s) if t in reading]
    top = m.predict_reading([[cc.EOS] + s[:i] for i in words], [reading[s[i]] for i in words], n=2, exact=True)
    for (ids, _lp), i in zip(top, words):
        assert (g[i, -1] < 2) == (s[i] in ids.tolist()), (name, i, g[i], ids)


@pytest.mark.parametrize("name", rc.GPU_MODELS)
def test_same_bits_however_the_rows_are_cut(name):
    m, got = model(name), ranks(name)
    seqs = rc.sequences(cc.MODELS[name][0])
    perm = [6, 2, 0, 5, 3, 1, 4]
    again = m.rank([seqs[i] for i in perm], cc.EOS)
    for j, i in enumerate(perm):
        assert np.array_equal(again[j], got[i]), (name, "permuted", i)
    for max_rows in (1, 3):
        again = m.rank(seqs, cc.EOS, max_rows=max_rows)
        assert all(np.array_equal(a, b) for a, b in zip(again, got)), (name, max_rows)
    only = m.rank(seqs, cc.EOS, readings=False)
    assert all(np.array_equal(o[:, 0], g[:, 0]) and o.shape[1] == 1 for o, g in zip(only, got))


@pytest.mark.parametrize("name", rc.GPU_MODELS)
def test_streams_and_carried_state(name):
    m = model(name)
    V = cc.MODELS[name][0]
    stream = np.random.RandomState(8).randint(0, V, size=(5, 13)).astype(np.int32)
    x, y = stream[:, :-1], stream[:, 1:]
    whole, h, c = m.rank_streams(x, y)
    a, h1, c1 = m.rank_streams(x[:, :5], y[:, :5])
    b, h2, c2 = m.rank_streams(x[:, 5:], y[:, 5:], h=h1, c=c1)
    assert np.array_equal(np.concatenate([a, b], axis=1), whole)
    assert torch.equal(h2.view(torch.int32), h.view(torch.int32)) and torch.equal(c2.view(torch.int32), c.view(torch.int32))
    rows = [3, 0, 4, 1, 2]
    again, _h, _c = m.rank_streams(x[rows], y[rows])
    assert np.array_equal(again, whole[rows])
    # a stream row is a sequence that starts with its first input
    seq = m.rank([list(y[r]) for r in range(5)], int(x[0, 0]))
    assert np.array_equal(seq[0], whole[0])
    # the state a ranking call returns is the state score_streams returns
    _nll, hs, cs = m.score_streams(x, y)
    assert torch.equal(hs.view(torch.int32), h.view(torch.int32)) and torch.equal(cs.view(torch.int32), c.view(torch.int32))


@pytest.mark.parametrize("name", ["tied", "dsoftmax", "tied-h512"])
def test_score_is_untouched_by_a_ranking_call(name):
    m = model(name)
    seqs = rc.sequences(cc.MODELS[name][0])
    before = m.score(seqs, cc.EOS)
    m.rank(seqs, cc.EOS)
    after = m.score(seqs, cc.EOS)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("name", ["small-vtable", "small-char"])
def test_perplexity_ranks_line(name, fx, capsys):
    """python -m jlm_amd.perplexity --ranks: one line behind the perplexity line, the metrics of rank() over the same tokens; without
    the option the output is the two lines it always was"""
    import os
    from jlm_amd import config as jconfig, perplexity, rank as R, synth
    from jlm_amd.data import CharVocab, Vocab
    f = fx(name)
    V = f["cfg"]["vocab_size"]
    synth.write_test_corpus(f["root"], f["lexicon"], V, 40, words_per_sentence=6, seed=13, oov_every=4)
    jconfig.set_root(f["root"])
    char = bool(f["cfg"].get("char_rnn"))
    vocab = (CharVocab if char else Vocab)(V)
    sents, _unk = perplexity.encode_lines(perplexity.read_lines(os.path.join(f["root"], "data", "test.txt")), vocab)
    base = ["--root", f["root"], "-e", "1", "--mode", "sentence"]
    perplexity.main(base)
    plain = capsys.readouterr().out.strip().split("\n")
    assert plain[-1].startswith("Test perplexity: ")            # (in front of it: the model's load line and the token count)
    perplexity.main(base + ["--ranks", "--top", "1,3", "--list", "4", "--max_prefix", "3"])
    out = capsys.readouterr().out.strip().split("\n")
    assert len(out) == len(plain) + 1 and out[-2] == plain[-1]
    from jlm_amd.model import LSTM_Model
    m = LSTM_Model(experiment_id=1)
    capsys.readouterr()
    rk = np.concatenate(m.rank(sents, vocab.t2i["<eos>"], readings=not char, max_prefix=3))
    targets = np.array([t for s in sents for t in s])
    assert out[-1] == perplexity.ranks_line(rk, targets, None if char else m.reading_index(), [1, 3], 4)
    acc = R.topk_accuracy(rk, [1, 3])
    assert out[-1].startswith("top-1: {:.4f}  top-3: {:.4f}  MRR: ".format(acc[1], acc[3])) and ("keystroke savings (list 4)" in out[-1]) == (not char)
    # stream mode ranks the corpus_iterator's tokens
    perplexity.main(["--root", f["root"], "-e", "1", "--mode", "stream", "-b", "4", "--num_steps", "5", "--ranks"])
    out = capsys.readouterr().out.strip().split("\n")
    from jlm_amd.score import stream_layout
    x, _y = stream_layout([i for s in sents for i in s], 4, 5)
    assert len(out) == len(plain) + 1 and "tokens: {} ranked".format(x.size) in out[-1]
