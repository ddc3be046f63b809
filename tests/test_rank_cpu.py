"""CPU: ranking the true next word (LSTM_Model.rank / rank_streams, jlm_amd/rank.py) -- the level table against
a brute-force scan of the readings, the host path end to end over the numpy double of the new ops (tests/fake_rank.py) against the
definition stated directly on the oracle's logits (tests/rank_cases.py), the metrics on hand-made ranks, every refusal, and the
condition that keeps the GPU comparison from being vacuous."""
import types

import numpy as np
import pytest

from jlm_amd import _lib, rank as R
from jlm_amd.readings import ReadingIndex
from tests import context_cases as cc
from tests import fake_rank
from tests import predict_cases as pc
from tests import rank_cases as rc


@pytest.fixture()
def fake(monkeypatch):
    return fake_rank.install(monkeypatch)


# ---------------------------------------------------------------------------------------------- the level table
def _index(entries):
    """a ReadingIndex over <unk>, <eos> and ``entries`` (display, reading)"""
    lex = [("<unk>", 0), ("<eos>", 9)] + [("%s/%s/N" % e, 1) for e in entries]
    return ReadingIndex(types.SimpleNamespace(lexicon=lex))


HAND = _index([("a", "ア"), ("b", "アイ"), ("c", "アイ"), ("d", "アイウ"), ("e", "カ"), ("f", "カキクケコサシ"), ("g", "アイ"), ("h", "イ"),
               ("i", "アイウエオカキクケコサシスセソタチツテトナニヌネノハヒフヘホマ"), ("j", "")])


def _check_table(index, max_prefix):
    off, lo, hi = index.level_table(max_prefix)
    assert off.dtype == lo.dtype == hi.dtype == np.int32 and len(off) == index.V + 1 and off[0] == 0 and off[-1] == len(lo) == len(hi)
    reading = {int(i): r for r, i in zip(index.readings, index.ids)}
    for w in range(index.V):
        a, b = int(off[w]), int(off[w + 1])
        if w not in reading:
            assert a == b                                                 # a word without a reading has no entries
            continue
        r = reading[w]
        want = rc.level_sets(index, w, max_prefix)[1:]
        want = [s for s in want[:-1] if s is not None] + [want[-1]]        # its prefix levels, then X
        assert b - a == min(len(r), max_prefix) + 2, (w, r)
        for e, S in zip(range(a, b), want):
            assert index.ids[lo[e]:hi[e]].tolist() == S.tolist(), (w, r, e - a)
        assert np.all(np.diff(lo[a:b]) >= 0) and np.all(np.diff(hi[a:b]) <= 0), (w, r)      # nested
        assert w in index.ids[lo[b - 1]:hi[b - 1]]


@pytest.mark.parametrize("max_prefix", [0, 1, 3, 8, 30])
def test_level_table_hand_lexicon(max_prefix):
    """a reading that is a prefix of another's, homophones, a one-kana reading, an empty reading token, readings longer than
    max_prefix (31 kana against 30), words without readings"""
    _check_table(HAND, max_prefix)
    off, lo, hi = HAND.level_table(max_prefix)
    w = 2 + 1                                                                # "b": アイ, homophones c and g
    assert HAND.ids[lo[off[w + 1] - 1]:hi[off[w + 1] - 1]].tolist() == [3, 4, 8]
    assert (lo[off[w]], hi[off[w]]) == (0, len(HAND))                         # level 0: every word that has a reading


@pytest.mark.parametrize("max_prefix", [0, 2, 8])
def test_level_table_synthetic_lexicon(max_prefix):
    _check_table(pc.index_of("tied"), max_prefix)                            # readings of 1 .. 4 kana: 2 is below the longest


@pytest.mark.parametrize("bad", [-1, 31, True, 2.0, None])
def test_level_table_refuses(bad):
    with pytest.raises(ValueError, match="max_prefix"):
        HAND.level_table(bad)


# ---------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("name", rc.GPU_MODELS)
def test_oracle_interval_is_mostly_one_rank(name):
    """the non-vacuity condition of tests/test_gpu_rank.py: at DELTA = 1e-4 the oracle's own interval is a single rank for at least
    80 % of the (token, level) entries of every model used there"""
    n = one = 0
    for lo, hi in rc.bounds(name):
        have = lo >= 0
        assert np.all(hi[have] >= lo[have])
        n += int(have.sum())
        one += int((have & (lo == hi)).sum())
    assert n >= 300 and one >= 0.8 * n, (name, one, n)


def test_interval_brackets_the_exact_rank():
    y = np.array([0.5, 0.50005, 0.49995, 2.0, -1.0, 0.5], dtype=np.float64)
    S = np.arange(6)
    assert rc.exact_rank(y, 0, S) == 2 and rc.exact_rank(y, 5, S) == 3       # the tie: lower id first
    assert rc.interval(y, 0, S) == (1, 4) and rc.interval(y, 3, S) == (0, 0)
    assert rc.exact_rank(y, 4, [4]) == 0 and rc.interval(y, 4, [4]) == (0, 0)


# ---------------------------------------------------------------------------------------------- the host path over the double
def _model(name):
    cc.set_root(name)
    from jlm_amd.model import LSTM_Model
    return LSTM_Model(experiment_id=1)


@pytest.mark.parametrize("name", rc.MODELS)
def test_rank_end_to_end(name, fake):
    m = _model(name)
    V = cc.MODELS[name][0]
    seqs = rc.sequences(V)
    got = m.rank(seqs, cc.EOS)
    assert [g.shape for g in got] == [(len(s), rc.MAX_PREFIX + 3) for s in seqs]
    rc.check_in_bounds(got, name)
    index = m.reading_index()
    for s, g in zip(seqs, got):
        for t, row in zip(s, g):
            n = rc.reading_len(index, t)
            want = np.array([True] + [n > 0 and j <= n for j in range(rc.MAX_PREFIX + 1)] + [n > 0])
            assert np.array_equal(row >= 0, want), (t, n, row)
            if n:
                assert row[0] >= row[1] >= row[1 + n] >= row[-1]              # nested sets: the rank cannot grow
    # chunked calls give the same bits, whatever the cut
    for max_rows in (1, 3):
        again = m.rank(seqs, cc.EOS, max_rows=max_rows)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), max_rows
    # column A alone, and a max_prefix below the longest reading
    only = m.rank(seqs, cc.EOS, readings=False)
    assert all(o.shape == (len(s), 1) and np.array_equal(o[:, 0], g[:, 0]) for o, g, s in zip(only, got, seqs))
    short = m.rank(seqs, cc.EOS, max_prefix=2)
    rc.check_in_bounds(short, name, max_prefix=2)
    assert all(np.array_equal(a[:, [0, 1, 2, 3, -1]], b[:, [0, 1, 2, 3, -1]]) for a, b in zip(short, got))


@pytest.mark.parametrize("name", ["tied", "untied"])
def test_rank_streams_and_carried_state(name, fake):
    import torch
    m = _model(name)
    V = cc.MODELS[name][0]
    rng = np.random.RandomState(5)
    stream = rng.randint(0, V, size=(3, 11)).astype(np.int32)
    x, y = stream[:, :-1], stream[:, 1:]
    whole, h, c = m.rank_streams(x, y)
    assert whole.shape == (3, 10, rc.MAX_PREFIX + 3) and whole.dtype == np.int32
    a, h1, c1 = m.rank_streams(x[:, :4], y[:, :4])
    b, h2, c2 = m.rank_streams(x[:, 4:], y[:, 4:], h=h1, c=c1)
    assert np.array_equal(np.concatenate([a, b], axis=1), whole)
    bits = lambda t: t.view(torch.int32).numpy()                      # (state rows may be split rows: compare the bits)
    assert np.array_equal(bits(h2), bits(h)) and np.array_equal(bits(c2), bits(c))
    # a stream row is a sequence that starts with its first input
    seq = m.rank([list(y[r]) for r in range(3)], int(x[0, 0]))
    assert np.array_equal(seq[0], whole[0])
    only, _h, _c = m.rank_streams(x, y, readings=False)
    assert np.array_equal(only[:, :, 0], whole[:, :, 0]) and only.shape == (3, 10, 1)
    empty, h0, c0 = m.rank_streams(x[:, :0], y[:, :0])
    assert empty.shape == (3, 0, rc.MAX_PREFIX + 3) and h0 is None and c0 is None


def test_double_flags(fake):
    """the double's two flag bits and its -1 rows, through the op layer the package calls"""
    import torch
    from jlm_amd import ops
    y = torch.tensor([[0.0, 1.0, float("nan"), 1.0], [0.0, 1.0, 2.0, 3.0], [3.0, 1.0, 2.0, 3.0]], dtype=torch.float32)
    rank = torch.full((3, 1), -7, dtype=torch.int32)
    flags = torch.zeros(1, dtype=torch.int32)
    ops.backend().rank_rows(y, 4, 4, 3, None, torch.tensor([2, 4, 3], dtype=torch.int32), None, None, None, None, 0, rank, flags)
    assert rank[:, 0].tolist() == [-1, -1, 1] and int(flags[0]) == 3
    with pytest.raises(RuntimeError):
        ops.backend().rank_rows(y, 4, 4, 3, None, torch.tensor([2, 4, 3], dtype=torch.int32), None, None, None, None, 33,
                                torch.zeros(3 * 34, dtype=torch.int32), flags)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(fake, fx):
    m = _model("tied")
    V = cc.MODELS["tied"][0]
    del fake.launches[:]
    for kw in (dict(sequences=[[1, 2], [3, V]]), dict(sequences=[[1, -1]]), dict(start=V), dict(start=-2),
               dict(max_prefix=-1), dict(max_prefix=31), dict(max_prefix=True), dict(max_prefix=1.5), dict(max_rows=0)):
        args = dict(sequences=[[2, 3]], start=cc.EOS)
        args.update(kw)
        with pytest.raises(ValueError):
            m.rank(**args)
    x = np.array([[2, 3, 4]])
    for a, kw in (((x, x[:, :2]), {}), ((x[0], x[0]), {}), ((x, x), dict(h=object())), ((x, np.array([[2, 3, V]])), {}),
                  ((x, x), dict(max_prefix=40))):
        with pytest.raises(ValueError):
            m.rank_streams(*a, **kw)
    import torch
    with pytest.raises(ValueError, match="carried state"):
        m.rank_streams(x, x, h=torch.zeros(2, 64), c=torch.zeros(2, 64))
    assert fake.launches == []
    assert m.rank([], cc.EOS) == [] and [g.shape for g in m.rank([[]], cc.EOS)] == [(0, rc.MAX_PREFIX + 3)]
    assert fake.launches == []


def test_character_model(fake, fx):
    """a character model ranks characters with readings=False; with readings it raises ReadingIndex's ValueError before any launch"""
    from jlm_amd import config as jconfig
    from jlm_amd.model import LSTM_Model
    jconfig.set_root(fx("small-char")["root"])
    m = LSTM_Model(experiment_id=1)
    del fake.launches[:]
    with pytest.raises(ValueError, match="character model"):
        m.rank([[2, 3]], 1)
    with pytest.raises(ValueError, match="character model"):
        m.rank_streams([[2, 3]], [[3, 4]])
    assert fake.launches == []
    got = m.rank([[2, 3, 4], [5]], 1, readings=False)
    assert [g.shape for g in got] == [(3, 1), (1, 1)] and all(np.all((g >= 0) & (g < m.dev.V)) for g in got)


def test_level_tables_are_cached_per_index_and_prefix(fake):
    m = _model("tied")
    rk = m._ranker()
    a = rk.levels(m.reading_index(), 8)
    assert rk.levels(m.reading_index(), 8) is a and rk.levels(m.reading_index(), 2) is not a
    assert a.n_levels == 10 and rk.levels(m.reading_index(), 2).n_levels == 4


# ---------------------------------------------------------------------------------------------- the metrics
#            A   j=0 j=1 j=2  X        (max_prefix = 2)
HAND_RANKS = np.array([[0, 0, 0, 0, 0],         # predicted before a key is typed: reading of 3 kana, costs 0
                       [7, 6, 2, 0, 0],         # list of 5: in the list after 1 kana (reading of 2)
                       [40, 30, 9, 5, 1],       # every level >= 5: costs its 4 kana
                       [3, -1, -1, -1, -1],     # no reading: excluded
                       [12, 9, 4, -1, 2],       # one-kana reading: in the list after its only kana: costs 1 of 1
                       [99, 50, 20, 4, 0]], dtype=np.int32)    # reading of 6 kana, max_prefix 2: in the list after 2
HAND_LENGTHS = [3, 2, 4, 0, 1, 6]


def test_metrics_on_hand_made_ranks():
    acc = R.topk_accuracy(HAND_RANKS, (1, 5, 10, 100))
    assert acc == {1: 1 / 6, 5: 2 / 6, 10: 3 / 6, 100: 1.0}
    assert R.mrr(HAND_RANKS) == pytest.approx((1 + 1 / 8 + 1 / 41 + 1 / 4 + 1 / 13 + 1 / 100) / 6, abs=1e-15)
    ks = R.keystrokes(HAND_RANKS, HAND_LENGTHS, 5)
    assert (ks["typed"], ks["kana"], ks["tokens"], ks["excluded"]) == (0 + 1 + 4 + 1 + 2, 16, 5, 1)
    assert ks["savings"] == pytest.approx(1 - 8 / 16, abs=1e-15)
    assert R.keystrokes(HAND_RANKS, HAND_LENGTHS, 1)["typed"] == 0 + 2 + 4 + 1 + 6        # a list of one
    hp = R.homophone_position(HAND_RANKS)
    assert hp == dict(mean=3 / 5, first=3 / 5, tokens=5)
    # a list of per-sequence arrays and a [B, n, columns] stream result are the same tokens
    parts = [HAND_RANKS[:2], HAND_RANKS[2:]]
    assert R.topk_accuracy(parts, (5,)) == {5: 2 / 6} and R.keystrokes(HAND_RANKS.reshape(2, 3, 5), HAND_LENGTHS, 5) == ks
    with pytest.raises(ValueError):
        R.keystrokes(HAND_RANKS[:, :1], HAND_LENGTHS, 5)
    with pytest.raises(ValueError):
        R.keystrokes(HAND_RANKS, HAND_LENGTHS[:-1], 5)
    with pytest.raises(ValueError):
        R.homophone_position(HAND_RANKS[:, :1])
    assert np.isnan(R.mrr(np.zeros((0, 1), dtype=np.int32)))
    assert R.reading_lengths(HAND).tolist() == [0, 0, 1, 2, 2, 3, 1, 7, 2, 1, 31, 1]


def test_lib_exposes_the_ranking_entries():
    import ctypes
    assert "jlm_rank_rows" in _lib.EXPORTS and "jlm_rank_frames" in _lib.EXPORTS
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "jlm_rank_rows") and hasattr(lib, "jlm_rank_frames")
    names = [f[0] for f in _lib.RankPlan._fields_]
    assert names[:2] == ["n_rows", "n_steps"] and names[-2:] == ["rank", "flags"] and "lv_off" in names
