"""GPU: ranking under the n-gram mixture end to end (LSTM_Model.rank_streams_ngram / rank_ngram; csrc jlm_rank_ngram_frames,
ngram_mix_rows_kernel) against the float64 yardstick of tests/ngram_mix_cases.py on the five models of tests/test_gpu_cache.py, orders
2 and 3: every device rank inside the oracle's interval over ``mixed_logits`` at delta = 2 DELTA + the derived bar of
tests/ngram_mix_budget.py, every cut of a stream bit for bit with ``tail`` carried, the lists against the oracle's order and log p,
one table that does not sum to one held to the row-normalised definition, and no result depending on what the call's buffers held."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd.ngram import NGramMix, estimate                                             # noqa: E402
from tests import ngram_mix_cases as nc, poison                                          # noqa: E402
from tests.gpu_rows import fixture_model, oracle_lm                                       # noqa: E402
from tests.test_gpu_cache import MODELS                                                   # noqa: E402

pytestmark = pytest.mark.gpu

TOP = 10
_ORACLE = {}


def oracle_logits(name, root, x):
    """the oracle's logits of the stream, computed once per model"""
    if name not in _ORACLE:
        _ORACLE[name] = nc.oracle_run(oracle_lm(root), x)
    return _ORACLE[name]


def run_cut(model, x, y, mix, cuts, top=TOP):
    h = c = tail = None
    parts, at = [], 0
    for k in cuts:
        res = model.rank_streams_ngram(x[:, at:at + k], y[:, at:at + k], mix, h, c, tail, max_prefix=nc.MAX_PREFIX, top=top)
        h, c, tail = res.h, res.c, res.tail
        parts.append(res)
        at += k
    return (np.concatenate([p.ranks for p in parts], axis=1), np.concatenate([p.top_ids for p in parts], axis=1),
            np.concatenate([p.top_logp for p in parts], axis=1), parts[-1])


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("name", MODELS)
def test_streams_rank_inside_the_oracles_interval(name, order, fx, monkeypatch):
    f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    sn = bool(m.self_norm)
    x, y = nc.stream(m.V)
    B, n = x.shape
    mix = nc.stream_table(x, y, m.V, order)
    ys = oracle_logits(name, f["root"], x)
    ymix, bars = nc.oracle_mixed(ys, x, mix, sn)
    assert nc.moved_share(ys, ymix, y) >= 0.1, name                          # the table matters
    plain = model.rank_streams(x, y, max_prefix=nc.MAX_PREFIX)[0]
    ranks, top_ids, top_logp, last = run_cut(model, x, y, mix, nc.CUTS[1])
    assert ranks.shape == (B, n, nc.MAX_PREFIX + 3) and ranks.dtype == np.int32 and top_ids.shape == top_logp.shape == (B, n, TOP)
    assert np.array_equal(last.tail, x[:, -2:])
    for cuts in (nc.CUTS[0], nc.CUTS[2]):                                    # every cut of the stream: the same bytes
        r2, i2, l2, l_ = run_cut(model, x, y, mix, cuts)
        assert np.array_equal(r2, ranks) and np.array_equal(i2, top_ids) and l2.tobytes() == top_logp.tobytes(), (name, cuts)
        assert torch.equal(l_.h.view(torch.int32), last.h.view(torch.int32)) and torch.equal(l_.c, last.c)
    single, total = nc.check_ranks(ranks, ymix, bars, y, model.reading_index(), name)
    nc.check_lists(top_ids, top_logp, ymix, bars, y, ranks, sn, mix.lam, name)
    print("%s order %d: %d / %d (token, level) intervals are a single rank; largest n-gram bar %.3e; ranks moved on %.0f %% of the positions" %
          (name, order, single, total, bars.max(), 100 * np.mean(ranks[:, :, 0] != plain[:, :, 0])))
    assert single >= 0.8 * total
    assert np.mean(ranks[:, :, 0] != plain[:, :, 0]) >= 0.1 and ranks[:, :, 0].mean() < plain[:, :, 0].mean()
    # the state the call leaves is rank_streams'; rank_streams is what it was
    again = model.rank_streams(x, y, max_prefix=nc.MAX_PREFIX)
    assert np.array_equal(again[0], plain) and torch.equal(again[1].view(torch.int32), last.h.view(torch.int32))


@pytest.mark.parametrize("name", ["small-tied", "small-tied-sn"])
def test_a_table_that_does_not_sum_to_one(name, fx, monkeypatch):
    """a file whose out-of-vocabulary n-grams were dropped: the ranks and the lists follow the row-normalised mixture, lse(y') - y'"""
    f, model = fixture_model(fx, name, monkeypatch)
    m = model.dev
    sn = bool(m.self_norm)
    x, y = nc.stream(m.V)
    leaky = nc.leaky_table(nc.stream_table(x, y, m.V, 3), m.V)
    assert np.exp(leaky.table.logq_all([int(x[0, 3]), int(x[0, 4])], m.V)).sum() < 0.9
    ys = oracle_logits(name, f["root"], x)
    ymix, bars = nc.oracle_mixed(ys, x, leaky, sn)
    res = model.rank_streams_ngram(x, y, leaky, max_prefix=nc.MAX_PREFIX, top=TOP)
    nc.check_ranks(res.ranks, ymix, bars, y, model.reading_index(), name)
    nc.check_lists(res.top_ids, res.top_logp, ymix, bars, y, res.ranks, sn, leaky.lam, name)


@pytest.mark.parametrize("name", ["small-vtable", "odd-tied"])
def test_rank_ngram_ragged_sequences(name, fx, monkeypatch):
    f, model = fixture_model(fx, name, monkeypatch)
    V = model.dev.V
    rng = np.random.RandomState(2)
    pool = rng.randint(2, V, size=6)
    seqs = [[int(w) for w in pool[rng.randint(0, 6, size=L)]] for L in (9, 0, 30, 1, 17, 0, 30)]
    mix = NGramMix(estimate(np.array([w for s in seqs for w in s + [nc.EOS]]), V, 3), 0.5)
    got = model.rank_ngram(seqs, nc.EOS, mix, max_prefix=nc.MAX_PREFIX)
    cut = model.rank_ngram(seqs, nc.EOS, mix, max_prefix=nc.MAX_PREFIX, max_rows=2)
    plain = model.rank(seqs, nc.EOS, max_prefix=nc.MAX_PREFIX)
    assert [g.shape for g in got] == [(len(s), nc.MAX_PREFIX + 3) for s in seqs]
    for s, g, g2 in zip(seqs, got, cut):
        assert np.array_equal(g, g2)
        if len(s):                                                          # a row alone, as a stream: the same ranks
            one = model.rank_streams_ngram(np.array([[nc.EOS] + s[:-1]]), np.array([s]), mix, max_prefix=nc.MAX_PREFIX)
            assert np.array_equal(one.ranks[0], g)
    assert any(np.any(g != p) for g, p in zip(got, plain))


@pytest.mark.parametrize("name", ["small-vtable", "odd-tied"])
def test_no_result_depends_on_what_a_buffer_held(name, fx, monkeypatch):
    """the logits' padding (odd-tied: ld_logits > V), the state rows and T under two fills: the same bytes"""
    f, model = fixture_model(fx, name, monkeypatch)
    x, y = nc.stream(model.dev.V, n=12)
    mix = nc.stream_table(x, y, model.dev.V, 3)

    def call():
        r = model.rank_streams_ngram(x, y, mix, max_prefix=nc.MAX_PREFIX, top=5)
        return [r.ranks, r.top_ids, r.top_logp, r.tail, r.h, r.c]
    poison.assert_same_three(call, what="rank_streams_ngram")


def test_refusals(fx, monkeypatch):
    f, model = fixture_model(fx, "small-tied", monkeypatch)
    V = model.dev.V
    x, y = nc.stream(V, n=6)
    mix = nc.stream_table(x, y, V, 3)
    for bad in (mix.table, None, "mix"):
        with pytest.raises(ValueError):
            model.rank_streams_ngram(x, y, bad)
    for kw in (dict(top=65), dict(top=-1), dict(tail=np.full((3, 2), V)), dict(tail=np.zeros((2, 2), dtype=np.int64)), dict(max_prefix=40)):
        with pytest.raises(ValueError):
            model.rank_streams_ngram(x, y, mix, **kw)
    with pytest.raises(ValueError):
        model.rank_ngram([[2, V]], nc.EOS, mix)
    empty = model.rank_streams_ngram(x[:, :0], y[:, :0], mix, top=3)
    assert empty.ranks.shape == (3, 0, 8 + 3) and empty.top_ids.shape == (3, 0, 3)


def test_perplexity_command_line_ranks_with_ngram(fx, tmp_path, capsys):
    """--ranks --ngram FILE prints a second --ranks line "with n-gram" over the same tokens, equal to the metrics of
    rank_streams_ngram over the same chunks with the tail carried; without --ngram the --ranks output is what it was"""
    from jlm_amd import config as jconfig, perplexity, rank as R
    from jlm_amd.data import Vocab
    from jlm_amd.ngram import NGramTable, write_srilm
    from jlm_amd.score import stream_layout
    from tests.gpu_rows import load_model
    f = fx("small-vtable")
    jconfig.set_root(f["root"])
    vocab = Vocab(f["cfg"]["vocab_size"])
    words = [w for w in vocab.w2i if w not in ("<unk>", "<eos>")]
    rng = np.random.RandomState(8)
    passage = " ".join(words[i] for i in rng.choice(len(words), size=29, replace=False))
    path, lm_path = str(tmp_path / "passage.txt"), str(tmp_path / "lm3")
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join([passage] * 12) + "\n")
    sents, _unk = perplexity.encode_lines(perplexity.read_lines(path), vocab)
    write_srilm(estimate(np.array([i for s in sents for i in s]), len(vocab), 3, eos=vocab.w2i["<eos>"]).rounded(), lm_path, vocab.i2w)
    args = ["--root", f["root"], "-e", "1", "--mode", "stream", "-b", "4", "--num_steps", "5", "--file", path, "--ranks"]
    perplexity.main(args)
    plain = [ln for ln in capsys.readouterr().out.splitlines() if "top-1:" in ln]
    perplexity.main(args + ["--ngram", lm_path, "--ngram-lam", "0.4"])
    out = [ln for ln in capsys.readouterr().out.splitlines() if "top-1:" in ln]
    assert len(plain) == 1 and len(out) == 2 and out[0] == plain[0] and out[1].startswith("with n-gram (order 3 lam 0.4): ")
    model = load_model(f["root"])
    mix = NGramMix(NGramTable.from_srilm(lm_path, vocab.t2i, 3), 0.4)
    x, y = stream_layout([i for s in sents for i in s], 4, 5)
    h = c = tail = None
    parts = []
    for i in range(x.shape[1] // 5):
        res = model.rank_streams_ngram(x[:, 5 * i:5 * i + 5], y[:, 5 * i:5 * i + 5], mix, h, c, tail)
        h, c, tail = res.h, res.c, res.tail
        parts.append(res.ranks)
    ranks = np.concatenate(parts, axis=1)
    want = perplexity.ranks_line(ranks.reshape(-1, ranks.shape[-1]), y.reshape(-1).astype(np.int64), model.reading_index(), [1, 5, 10], 5)
    assert out[1] == "with n-gram (order 3 lam 0.4): " + want
    mrr = lambda line: float(line.split("MRR: ")[1].split()[0])
    assert mrr(out[1]) > mrr(out[0])                                       # the table was counted from this very passage
    assert R.mrr(ranks) == pytest.approx(mrr(out[1]), abs=1e-4)
