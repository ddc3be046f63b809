"""CPU: ranking, prediction and completion under the n-gram mixture (LSTM_Model.rank_streams_ngram / rank_ngram and the ``ngram=`` of
predict_top / predict_reading / complete / complete_reading; jlm_amd/ngram.py, jlm_amd/ngram_mix.py) -- the table
layout of the row walk against ``logq_all``, ``mixed_logits`` against its definition, the host path of all six entry points end to end
over the numpy double (tests/fake_ngram_mix.py) against the float64 yardstick of tests/ngram_mix_cases.py, every refusal, ``ngram=None``
calling what it called before, and the condition that keeps the comparison from passing by ignoring the table."""
import numpy as np
import pytest

from jlm_amd import _lib
from jlm_amd.ngram import MIX_MAX_V, SUCCESSOR_TENSORS, NGramMix, NGramTable, check_mix_rows, estimate, mixed_logits, pack, successor_tensors
from tests import context_cases as cc
from tests import fake_ngram_mix
from tests import ngram_mix_cases as nc
from tests import rank_cases as rc
from tests.gpu_rows import ragged_prompts

MAX_PREFIX = nc.MAX_PREFIX


@pytest.fixture()
def fake(monkeypatch):
    return fake_ngram_mix.install(monkeypatch)


def _model(name):
    cc.set_root(name)
    from jlm_amd.model import LSTM_Model
    return LSTM_Model(experiment_id=1)


def _struct(table, V):
    import torch
    tens, arr = successor_tensors(table, V, torch.device("cpu"))
    return fake_ngram_mix.rows_struct([tens[k] for k in SUCCESSOR_TENSORS],
                                      [arr["bi_w"].size, arr["tri_w"].size, arr["n_ctx"], arr["log2cap"], arr["max_probe"]]), tens


def _walk_equals_logq(table, V, hists):
    st, _keep = _struct(table, V)
    n = 0
    for u, v in hists:
        for order in range(1, table.order + 1):
            h = [] if order < 2 or v < 0 else [v] if order < 3 or u < 0 else [u, v]
            q = table.logq_all(h, V)                                        # (a lower order: a shorter history of the same table)
            w = fake_ngram_mix.walk(st, V, u, v, order).astype(np.float64)
            assert np.array_equal(np.isfinite(q), np.isfinite(w)), (u, v, order)
            ok = np.isfinite(q)
            # two float32 additions of values the table holds exactly: 2^-23 of the largest partial sum
            assert np.all(np.abs(q[ok] - w[ok]) <= 2.0 ** -22 * (1.0 + np.abs(q[ok]))), (u, v, order)
            n += int(ok.sum())
    return n


# ---------------------------------------------------------------------------------------------- the table layout
@pytest.mark.parametrize("order", [1, 2, 3])
def test_successor_arrays_reproduce_logq_all_on_estimated_tables(order):
    rng = np.random.RandomState(order)
    V = 40
    ids = rng.randint(2, V, size=500)
    ids[::11] = 1
    table = estimate(ids, V, order).rounded()
    hists = [(-1, -1)] + [(-1, v) for v in range(0, V, 3)] + [(int(u), int(v)) for u, v in rng.randint(0, V, size=(60, 2))] + \
        [(int(ids[i]), int(ids[i + 1])) for i in range(0, 60, 2)]
    assert _walk_equals_logq(table, V, hists) > 1000
    arr = table.successor_arrays(V)
    assert arr is table.successor_arrays(V)                                 # memoised per V
    assert arr["uni_lp"].dtype == arr["bi_lp"].dtype == arr["tri_bow"].dtype == np.float32 and arr["bi_off"].dtype == np.int32
    assert arr["bi_off"].shape == (V + 1,) and arr["tri_off"].shape == (arr["n_ctx"] + 1,) and arr["ctx_keys"].dtype == np.uint64
    again = NGramTable(table.keys, table.lp, table.bow, order).successor_arrays(V)
    for k, a in arr.items():                                                # the bytes are deterministic
        assert (a.tobytes() == again[k].tobytes()) if isinstance(a, np.ndarray) else a == again[k], k
    wider = table.successor_arrays(V + 7)                                   # another V: its own arrays, the extra words without a unigram
    assert wider["uni_lp"].shape == (V + 7,) and np.all(np.isneginf(wider["uni_lp"][V:])) and wider["bi_off"][-1] == arr["bi_off"][-1]


def test_successor_arrays_on_a_hand_made_table():
    table = nc.handmade_table()
    V = 8
    arr = table.successor_arrays(V)
    assert np.isneginf(arr["uni_lp"][7]) and arr["uni_bow"][1] == 0 and arr["uni_bow"][6] == np.float32(-0.75)
    assert arr["bi_off"].tolist() == [0, 0, 0, 2, 3, 4, 5, 5, 5] and arr["bi_w"].tolist() == [2, 3, 0, 5, 1]
    # contexts: (2, 2) and (2, 3) carry a weight -- (2, 3) without successors --, (4, 5) has successors and no weight
    ctx = sorted(((2, 2), (2, 3), (4, 5)), key=lambda c: pack(c))
    assert arr["n_ctx"] == 3 and arr["tri_off"].tolist() == [0, 1, 1, 3]
    assert arr["tri_bow"].tolist() == [np.float32(-0.0625), np.float32(-0.375), 0.0] and arr["tri_w"].tolist() == [3, 0, 7]
    st, _keep = _struct(table, V)
    assert [fake_ngram_mix.context_index(st, u, v) for u, v in ctx] == [0, 1, 2] and fake_ngram_mix.context_index(st, 3, 0) == -1
    hists = [(-1, -1)] + [(u, v) for u in range(-1, V) for v in range(-1, V)]
    assert _walk_equals_logq(table, V, hists) > 1000
    q = table.logq_all([4, 5], V)
    assert q[7] == -1.5 and q[0] == -0.5 and q[1] == -1.0 and np.isneginf(table.logq_all([2, 3], V)[7])
    assert table.logq_all([2, 3], V)[0] == pytest.approx(-0.375 - 0.75)     # bow(2 3), then the bigram (3, 0)
    assert table.logq_all([0, 6], V)[2] == pytest.approx(-0.75 - 1.0)       # a word with a weight and no successor at all
    with pytest.raises(ValueError):
        table.successor_arrays(7)                                           # word id 7 >= V
    with pytest.raises(ValueError):
        table.successor_arrays(0)


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("self_norm", [False, True])
def test_mixed_logits_is_the_mixture(self_norm):
    rng = np.random.RandomState(5)
    table = nc.handmade_table()
    V, lam = 8, 0.3
    for hist in ([], [5], [4, 5], [2, 3], [-1, 5], [7, -1], [0, 6]):
        y = 2.0 * rng.standard_normal(V)
        if self_norm:
            y -= np.log(np.exp(y).sum()) + 0.05
        y[0] = -np.inf                                                      # the model gives word 0 no mass
        clean = [w for w in hist]
        gaps = [i for i, w in enumerate(clean) if w < 0]
        clean = clean[gaps[-1] + 1:] if gaps else clean
        q = table.logq_all(clean, V)
        L = 0.0 if self_norm else np.log(np.exp(y).sum())
        got = mixed_logits(table, hist, y, lam, self_norm)
        p = (1 - lam) * np.exp(y - L) + lam * np.exp(q)
        assert np.allclose((1 - lam) * np.exp(got - L), p, rtol=1e-12, atol=0)
        assert got[~np.isfinite(q)].tobytes() == y[~np.isfinite(q)].tobytes()          # q = -inf: the same bits
        assert np.isfinite(got[0]) and got[0] == pytest.approx(L + np.log(lam / (1 - lam)) + q[0])
        if not self_norm:                                                   # the selection kernels' report: the row-normalised mixture
            Z = np.exp(q).sum()
            lse = np.log(np.exp(got).sum())
            assert np.allclose(lse - got, -np.log(p / ((1 - lam) + lam * Z)), rtol=0, atol=1e-12)
    for lam in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            mixed_logits(table, [], np.zeros(V), lam)


def test_estimated_tables_sum_to_one_and_a_leaky_one_does_not():
    x, y = nc.stream(600)
    mix = nc.stream_table(x, y, 600, 3)
    leaky = nc.leaky_table(mix, 600)
    for h in ([], [int(x[0, 3])], [int(x[0, 3]), int(x[0, 4])]):
        assert abs(np.exp(mix.table.logq_all(h, 600)).sum() - 1.0) < 1e-5                # (the float32 rounding of the values)
        assert np.exp(leaky.table.logq_all(h, 600)).sum() < 0.9


# ---------------------------------------------------------------------------------------------- the host path over the double
def _run_cut(m, x, y, mix, cuts, top=5):
    h = c = tail = None
    parts, at = [], 0
    for k in cuts:
        res = m.rank_streams_ngram(x[:, at:at + k], y[:, at:at + k], mix, h, c, tail, max_prefix=MAX_PREFIX, top=top)
        h, c, tail = res.h, res.c, res.tail
        parts.append(res)
        at += k
    return (np.concatenate([p.ranks for p in parts], axis=1), np.concatenate([p.top_ids for p in parts], axis=1),
            np.concatenate([p.top_logp for p in parts], axis=1), parts[-1])


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("name", rc.MODELS)
def test_rank_streams_ngram_end_to_end(name, order, fake):
    m = _model(name)
    V = cc.MODELS[name][0]
    x, y = nc.stream(V)
    B, n = x.shape
    mix = nc.stream_table(x, y, V, order)
    plain = m.rank_streams(x, y, max_prefix=MAX_PREFIX)[0]
    ranks, ids, logp, last = _run_cut(m, x, y, mix, nc.CUTS[1])
    assert ranks.shape == plain.shape and ranks.dtype == np.int32 and ids.shape == logp.shape == (B, n, 5)
    assert np.array_equal(last.tail, x[:, -2:])
    for cuts in (nc.CUTS[0], nc.CUTS[2]):
        r2, i2, l2, _ = _run_cut(m, x, y, mix, cuts)
        assert np.array_equal(r2, ranks) and np.array_equal(i2, ids) and l2.tobytes() == logp.tobytes(), cuts
    lm = cc.oracle(name).model
    sn = bool(lm.config["self_norm"])
    ys = nc.oracle_run(lm, x)
    ymix, bars = nc.oracle_mixed(ys, x, mix, sn)
    single, total = nc.check_ranks(ranks, ymix, bars, y, m.reading_index(), name)
    assert total >= 300 and single >= 0.8 * total, (name, single, total)
    nc.check_lists(ids, logp, ymix, bars, y, ranks, sn, mix.lam, name)
    # the table matters: at lam = 0.5 the exact mixed rank differs from the plain one on a tenth of the positions or more
    assert nc.moved_share(ys, ymix, y) >= 0.1, name
    assert np.mean(ranks[:, :, 0] != plain[:, :, 0]) >= 0.1 and ranks[:, :, 0].mean() < plain[:, :, 0].mean()
    assert np.array_equal(m.rank_streams(x, y, max_prefix=MAX_PREFIX)[0], plain)          # rank_streams is what it was
    # readings=False: column A alone, the same ranks
    only_a = m.rank_streams_ngram(x, y, mix, readings=False)
    assert only_a.ranks.shape == (B, n, 1) and np.array_equal(only_a.ranks[:, :, 0], ranks[:, :, 0]) and only_a.top_ids is None


def test_rank_ngram_ragged_sequences(fake):
    m = _model("tied")
    V = cc.MODELS["tied"][0]
    rng = np.random.RandomState(2)
    pool = rng.randint(2, V, size=6)
    seqs = [[int(w) for w in pool[rng.randint(0, 6, size=L)]] for L in (9, 0, 30, 1, 17, 0, 30)]
    ids = [w for s in seqs for w in s + [cc.EOS]]
    mix = NGramMix(estimate(np.array(ids), V, 3), 0.5)
    got = m.rank_ngram(seqs, cc.EOS, mix, max_prefix=MAX_PREFIX)
    cut = m.rank_ngram(seqs, cc.EOS, mix, max_prefix=MAX_PREFIX, max_rows=2)
    plain = m.rank(seqs, cc.EOS, max_prefix=MAX_PREFIX)
    assert [g.shape for g in got] == [(len(s), MAX_PREFIX + 3) for s in seqs]
    lm = cc.oracle("tied").model
    total = 0
    for s, g, g2 in zip(seqs, got, cut):
        assert np.array_equal(g, g2)
        if len(s):                                                          # the history at step t is (start, s[0 .. t - 1])
            x1, y1 = np.array([[cc.EOS] + s[:-1]]), np.array([s])
            one = m.rank_streams_ngram(x1, y1, mix, max_prefix=MAX_PREFIX)
            assert np.array_equal(one.ranks[0], g)
            # ... and the float64 yardstick: the oracle's logits of the row, mixed under those histories
            ymix, bars = nc.oracle_mixed(nc.oracle_run(lm, x1), x1, mix, bool(lm.config["self_norm"]))
            total += nc.check_ranks(g[None], ymix, bars, y1, m.reading_index(), "rank_ngram")[1]
    assert total >= 300
    assert any(np.any(g != p) for g, p in zip(got, plain))


@pytest.mark.parametrize("name", rc.MODELS)
def test_predict_and_complete_under_the_mixture(name, fake):
    m = _model(name)
    V = cc.MODELS[name][0]
    lm = cc.oracle(name).model
    x, y = nc.stream(V, seed=4)
    mix = nc.stream_table(x, y, V, 3)
    words = np.unique(x)
    rng = np.random.RandomState(8)
    prompts = [[cc.EOS] + [int(w) for w in words[rng.randint(0, len(words), size=k)]] for k in (2, 0, 1, 4, 3)]
    # predict_top / predict_reading
    top = m.predict_top(prompts, n=7, ngram=mix)
    assert nc.check_top(top, lm, mix, prompts, 7, tag=name) >= 20
    plain = m.predict_top(prompts, n=7)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(top, plain))                # the table moves the lists
    index = m.reading_index()
    kana = [index.readings[int(np.flatnonzero(index.ids == int(words[i]))[0])][:1] for i in range(len(prompts))]
    sets = [index.lookup(r) for r in kana]
    rd = m.predict_reading(prompts, kana, n=5, ngram=mix)
    assert nc.check_top(rd, lm, mix, prompts, 5, sets=sets, tag=name + " reading") >= 10
    # complete / complete_reading: the oracle on the device's own beams
    comp = m._completer()
    for B in (1, 5):
        N = 3
        order = np.argsort(-np.array([len(p) for p in prompts]), kind="stable")
        bp_parent, bp_word, bp_nll, score = comp.run([np.asarray(prompts[i]) for i in order], N, B, ngram=mix)
        agree = amb = 0
        for p, i in enumerate(order):
            a, b = nc.oracle_follow(lm, mix, prompts[i], bp_parent, bp_word, bp_nll, score, p, N, B)
            agree, amb = agree + a, amb + b
        assert amb <= max(1, (agree + amb) // 20), (name, B, agree, amb)
        res = m.complete(prompts, N, beam_width=B, ngram=mix)
        shift = -np.log1p(-0.5) if lm.config["self_norm"] else 0.0
        for p, i in enumerate(order):
            for r, (ids, nll, tot) in enumerate(res[i]):
                assert len(ids) == N and tot == pytest.approx(score[p * B + r] + N * shift, abs=1e-9) and nll.sum() == pytest.approx(tot, abs=1e-9)
    # the masked first frame under the mixture, against the same yardstick: a set of every second word, and complete_reading's sets
    order = np.argsort(-np.array([len(p) for p in prompts]), kind="stable")
    big = [np.arange(0, V, 2)] * len(prompts)
    for first, B in ((big, 4), ([sets[i] if len(sets[i]) > 3 else None for i in range(len(prompts))], 3)):
        bp_parent, bp_word, bp_nll, score = comp.run([np.asarray(prompts[i]) for i in order], 2, B, first_sets=[first[i] for i in order], ngram=mix)
        for p, i in enumerate(order):
            nc.oracle_follow(lm, mix, prompts[i], bp_parent, bp_word, bp_nll, score, p, 2, B, first_set=first[i])
    res = m.complete(prompts, 2, beam_width=4, first_allowed=big, ngram=mix)
    assert all(len(r) == 4 and all(h[0][0] % 2 == 0 for h in r) for r in res)
    same = m.complete_reading(prompts, kana, 2, beam_width=3, ngram=mix)
    shift = -np.log1p(-0.5) if lm.config["self_norm"] else 0.0
    bp_parent, bp_word, bp_nll, score = comp.run([np.asarray(prompts[i]) for i in order], 2, 3, first_sets=[sets[i] for i in order], ngram=mix)
    for p, i in enumerate(order):                                          # complete_reading is that call, read back
        assert all(int(h[0][0]) in set(sets[i].tolist()) for h in same[i])
        fin = [r for r in range(3) if np.isfinite(score[p * 3 + r])]
        assert [h[2] for h in same[i]] == pytest.approx([score[p * 3 + r] + 2 * shift for r in fin], abs=1e-9)


def test_ngram_none_calls_what_it_called_before(fake):
    m = _model("tied")
    V = cc.MODELS["tied"][0]
    prompts = ragged_prompts(4, V, seed=3)
    x, y = nc.stream(V)
    mix = nc.stream_table(x, y, V, 3)
    calls = []
    for kw in ({}, dict(ngram=None)):
        del fake.launches[:]
        top = m.predict_top(prompts, n=4, **kw)
        hyps = m.complete(prompts, 2, beam_width=3, **kw) + m.complete(prompts, 2, beam_width=3, first_allowed=[np.arange(5, 50)] * 4, **kw)
        calls.append((top, hyps, [l for l in fake.launches if l.startswith("complete_frames")]))
    assert calls[0][2] == calls[1][2] == ["complete_frames", "complete_frames", "complete_frames_masked"]
    for (ia, la), (ib, lb) in zip(calls[0][0], calls[1][0]):
        assert np.array_equal(ia, ib) and la.tobytes() == lb.tobytes()
    for ra, rb in zip(calls[0][1], calls[1][1]):
        assert len(ra) == len(rb)
        for (ia, na, ta), (ib, nb, tb) in zip(ra, rb):
            assert np.array_equal(ia, ib) and na.tobytes() == nb.tobytes() and ta == tb
    del fake.launches[:]
    m.complete(prompts, 2, beam_width=3, ngram=mix)
    m.complete(prompts, 2, beam_width=3, first_allowed=[np.arange(5, 50)] * 4, ngram=mix)
    assert [l for l in fake.launches if l.startswith("complete_frames")] == ["complete_frames_ngram"] * 2
    assert "ngram_hist_advance" in fake.launches and "ngram_mix_rows" in fake.launches
    del fake.launches[:]
    m.predict_top(prompts, n=4, ngram=mix)                                  # one word: no history to carry
    assert "ngram_hist_advance" not in fake.launches and "ngram_mix_rows" in fake.launches


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(fake):
    import torch
    m = _model("tied")
    V = cc.MODELS["tied"][0]
    x, y = nc.stream(V, n=6)
    mix = nc.stream_table(x, y, V, 3)
    prompts = ragged_prompts(3, V, seed=1)
    m.rank_streams_ngram(x, y, mix, readings=False)
    del fake.launches[:]
    too_wide = NGramMix(NGramTable([pack((V,))], [-1.0], [0.0], 1), 0.5)     # a word id the model does not have
    for bad in (mix.table, "mix", None, too_wide):
        with pytest.raises(ValueError):
            m.rank_streams_ngram(x, y, bad, readings=False)
        with pytest.raises(ValueError):
            m.rank_ngram([[2, 3]], cc.EOS, bad, readings=False)
    for bad in (mix.table, "mix", too_wide):
        with pytest.raises(ValueError):
            m.predict_top(prompts, n=3, ngram=bad)
        with pytest.raises(ValueError):
            m.complete(prompts, 2, beam_width=3, ngram=bad)
        with pytest.raises(ValueError):
            m.complete_reading(prompts, ["a"] * 3, 2, beam_width=3, ngram=bad)
        with pytest.raises(ValueError):
            m.predict_reading(prompts, ["a"] * 3, n=3, ngram=bad)
    for lam in (0.0, 1.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            NGramMix(mix.table, lam)
    with pytest.raises(ValueError, match="at most %d words" % MIX_MAX_V):
        check_mix_rows(mix, MIX_MAX_V + 1)
    assert check_mix_rows(mix, 262144) is mix
    for a, kw in (((x, y[:, :2]), {}), ((x[0], y[0]), {}), ((x, np.full_like(y, V)), {}), ((x, y), dict(top=65)), ((x, y), dict(top=-1)),
                  ((x, y), dict(top=1.5)), ((x, y), dict(tail=np.zeros((2, 2), dtype=np.int64))), ((x, y), dict(tail=np.zeros((3, 2)))),
                  ((x, y), dict(tail=np.full((3, 2), V))), ((x, y), dict(tail=np.full((3, 2), -2))),
                  ((x, y), dict(h=torch.zeros(3, m.dev.H))), ((x, y), dict(max_prefix=40, readings=True))):
        args = dict(readings=False)
        args.update(kw)
        with pytest.raises(ValueError):
            m.rank_streams_ngram(*a, mix, **args)
    with pytest.raises(ValueError):
        m.rank_ngram([[2, V]], cc.EOS, mix)
    assert fake.launches == []
    empty = m.rank_streams_ngram(x[:, :0], y[:, :0], mix, tail=np.full((3, 2), 5), top=3)
    assert empty.ranks.shape == (3, 0, rc.MAX_PREFIX + 3) and empty.top_ids.shape == (3, 0, 3) and np.all(empty.tail == 5)
    assert m.rank_ngram([], cc.EOS, mix) == [] and fake.launches == []


def test_double_refuses_what_the_header_refuses(fake):
    """the launchers' -1 cases through the double, as tests/test_gpu_ngram_mix_rows.py asks them of the library"""
    table = nc.handmade_table()
    V = 8
    st, _keep = _struct(table, V)
    y = np.zeros((2, 8), dtype=np.float32)
    hist = np.array([[4, 5], [-1, 3]], dtype=np.int32)
    a = lambda v: v.ctypes.data
    base = dict(y=a(y), ld_y=8, n_cols=V, self_norm=0, table=st, hist=a(hist), n_rows=2, n_dev=None, lam=0.5, order=3, flags=None, stream=None)
    for kw in (dict(order=0), dict(order=4), dict(lam=0.0), dict(lam=1.0), dict(y=None), dict(hist=None), dict(n_rows=-1), dict(ld_y=6),
               dict(ld_y=9), dict(n_cols=0), dict(n_cols=MIX_MAX_V + 1, ld_y=MIX_MAX_V + 4), dict(table=None), dict(hist=a(hist) + 2)):
        assert fake.jlm_ngram_mix_rows(**dict(base, **kw)) == -1, kw
    for field, bad in (("n_bi", -1), ("n_tri", -1), ("n_ctx", -1), ("log2cap", 5), ("max_probe", -1), ("uni_lp", None), ("ctx_keys", None)):
        st2, _k2 = _struct(table, V)
        setattr(st2, field, bad)
        assert fake.jlm_ngram_mix_rows(**dict(base, table=st2)) == -1, field
    assert fake.launches == [] and not y.any() and fake.jlm_ngram_mix_rows(**dict(base, n_rows=0)) == 0 and fake.launches == []
    assert fake.jlm_ngram_mix_rows(**base) == 0 and y.any()
    hin, out = np.array([[1, 2], [3, 4]], dtype=np.int32), np.zeros((3, 2), dtype=np.int32)
    prev, word = np.array([1, 0, 5], dtype=np.int32), np.array([7, 6, 5], dtype=np.int32)
    assert fake.jlm_ngram_hist_advance(a(hin), 2, a(prev), a(word), 3, a(out), None) == 0
    assert out.tolist() == [[4, 7], [2, 6], [-1, 5]]
    for kw in (dict(n=-1), dict(hist_in=None), dict(hist_out=a(hin)), dict(word=None)):
        args = dict(hist_in=a(hin), n_in=2, prev_row=a(prev), word=a(word), n=3, hist_out=a(out), stream=None)
        args.update(kw)
        assert fake.jlm_ngram_hist_advance(**args) == -1, kw


def test_new_entry_points_in_ctypes_table():
    for n in ("jlm_ngram_mix_rows", "jlm_ngram_mix_refuse", "jlm_ngram_hist_advance", "jlm_rank_ngram_frames", "jlm_complete_frames_ngram"):
        assert n in _lib.EXPORTS
    assert [f[0] for f in _lib.NgramRows._fields_][:3] == ["uni_lp", "uni_bow", "bi_off"]
    lib = _lib.lib()
    assert lib.jlm_abi_version() == 12 and hasattr(lib, "jlm_ngram_mix_rows")
