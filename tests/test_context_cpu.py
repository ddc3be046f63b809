"""CPU: the host side of decoding with a left context (jlm_amd/context.py) and the yardstick its GPU tests use
(tests/context_cases.py): the primed-oracle proxy against the chain rule, context normalisation and its errors, the priming plan's
arrays against a brute-force restatement, the eval harness's sentence split."""
import types

import numpy as np
import pytest

from jlm_amd import context as jctx
from tests import context_cases as cc


# ---------------------------------------------------------------------------------------------- the yardstick checks itself
@pytest.mark.parametrize("name", ["tied", "vtable"])
def test_primed_oracle_is_the_chain_rule(name):
    """the 1-best score of the unmodified oracle behind the proxy = the sum of -log p(word | [<eos>] + context + earlier words) along
    its path, to 1e-9, on all 12 inputs; and the context changes the result"""
    o = cc.oracle(name)
    V = cc.MODELS[name][0]
    changed = 0
    for text, ctx in zip(cc.sentences(), cc.contexts(V)):
        got = cc.primed_decode(o, text, ctx, beam_width=5)
        score, words = got[0]
        want = cc.chain_nll(o.model, [cc.EOS] + cc.ids_of(ctx), cc.path_ids(o, words)).sum()
        assert abs(score - want) <= 1e-9, (name, text, ctx, score, want)
        if cc.ids_of(ctx):
            plain = o.decode(text, beam_width=5)
            changed += [x for x in plain] != [x for x in got]
        else:
            assert o.decode(text, beam_width=5) == got          # an empty context is the oracle's own decode
    assert changed >= 8, changed


def test_primed_lm_forwards_everything_but_the_root():
    o = cc.oracle("tied")
    p = cc.PrimedLM(o.model, [cc.EOS, 7, 9])
    h, c = p.zero_state(1)
    hw, cw = cc.oracle_state(o.model, [cc.EOS, 7])
    assert np.array_equal(h, hw) and np.array_equal(c, cw)
    a = p.predict([cc.EOS], h, c)
    b = o.model.predict([9], h, c)
    assert np.array_equal(a[0], b[0])
    a2 = p.predict([5, 6], np.repeat(h, 2, 0), np.repeat(c, 2, 0))         # later calls pass through
    b2 = o.model.predict([5, 6], np.repeat(h, 2, 0), np.repeat(c, 2, 0))
    assert np.array_equal(a2[0], b2[0])
    assert p.config is o.model.config


# ---------------------------------------------------------------------------------------------- normalisation
def test_normalize_contexts():
    w2i = {"<unk>": 0, "<eos>": 1, "a/a": 5, "b/b": 6}
    got = jctx.normalize_contexts([None, [], [5, np.int64(6)], ["a/a", "zz/zz", 6], (1, 1)], 10, w2i, unk=0)
    assert [g.tolist() for g in got] == [[], [], [5, 6], [5, 0, 6], [1, 1]]
    assert all(g.dtype == np.int64 for g in got)


@pytest.mark.parametrize("bad", [[[10]], [[-1]], [[3, 99]], [["a/a"]], [[1.5]], [[True]], ["ab"], None, "abc", 3])
def test_normalize_contexts_errors(bad):
    with pytest.raises(ValueError):
        jctx.normalize_contexts(bad, 10)           # (no w2i: a string is an error here)


def test_resolve_errors_before_anything_runs():
    model = types.SimpleNamespace(dev=types.SimpleNamespace(V=10), prime=lambda ctxs: pytest.fail("primed"))
    w2i = {"<unk>": 0, "<eos>": 1}
    assert jctx.resolve(model, None, 3, w2i) is None
    assert jctx.resolve(model, [None, [], ()], 3, w2i) is None              # nothing but empty entries: today's decode, no priming
    assert jctx.resolve(model, [], 1, w2i, single=True) is None
    with pytest.raises(ValueError):
        jctx.resolve(model, [[2]], 2, w2i)                                   # one entry per input
    with pytest.raises(ValueError):
        jctx.resolve(model, [[2], [10]], 2, w2i)                             # id outside [0, V)
    with pytest.raises(ValueError):
        jctx.resolve(model, "ab", 2, w2i)
    other = jctx.ContextState(object(), None, None, None, None, [1, 1], [0, 0])
    with pytest.raises(ValueError):
        jctx.resolve(model, other, 2, w2i)                                   # a state of another model
    same = jctx.ContextState(model.dev, None, None, None, None, [1, 1], [0, 0])
    with pytest.raises(ValueError):
        jctx.resolve(model, same, 3, w2i)                                    # one row per input
    assert jctx.resolve(model, same, 2, w2i) is None                         # every history <eos> alone
    seeded = jctx.ContextState(model.dev, None, None, None, None, [1, 4], [0, 0])
    d = jctx.resolve(model, seeded, 2, w2i)
    assert d.rows == [0, 1] and d.sub([1]).rows == [1] and d.sub([1]).state is seeded


# ---------------------------------------------------------------------------------------------- the priming plan
def _contexts(lengths, V=50, seed=3):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, V, size=L).astype(np.int64) for L in lengths]


@pytest.mark.parametrize("max_rows", [8, 2, 1])
def test_priming_plan_against_brute_force(max_rows):
    """lengths 0, 1, 7, 7, 40 (one row never steps): every array restated element by element, then the plan RUN with a toy recurrence
    (a row's state = the words it consumed) over two ping-pong sets -- every stepped row ends as hist[:-1]"""
    lengths = [7, 0, 40, 1, 7]
    ctxs = _contexts(lengths)
    hist = [[cc.EOS] + c.tolist() for c in ctxs]
    chunks = jctx.plan_priming(ctxs, max_rows)
    order = sorted(range(len(ctxs)), key=lambda i: -lengths[i])             # stable, longest first
    assert [int(i) for ch in chunks for i in ch["idx"]] == order
    assert all(len(ch["idx"]) <= max_rows for ch in chunks)
    for ch in chunks:
        idx = [int(i) for i in ch["idx"]]
        R, S = len(idx), ch["n_steps"]
        assert S == lengths[idx[0]]
        assert ch["word"].shape == (S, R) and ch["prev"].shape == (S, R) and len(ch["n_live"]) == S
        assert ch["word"].dtype == np.int32 and ch["prev"].dtype == np.int32
        assert ch["last"].tolist() == [hist[i][-1] for i in idx]
        assert ch["has"].tolist() == [int(lengths[i] > 0) for i in idx]
        sets = [[None] * R, [None] * R]
        for f in range(S):
            live = [r for r in range(R) if f >= S - lengths[idx[r]]]
            assert live == list(range(int(ch["n_live"][f])))                 # the live rows are a prefix
            for r in live:
                k = f - (S - lengths[idx[r]])
                assert ch["word"][f, r] == hist[idx[r]][k]
                assert ch["prev"][f, r] == (-1 if k == 0 else r)
                src = [] if ch["prev"][f, r] < 0 else sets[f % 2][ch["prev"][f, r]]
                sets[(f + 1) % 2][r] = src + [int(ch["word"][f, r])]
        for r in range(R):
            if lengths[idx[r]]:
                assert sets[S % 2][r] == hist[idx[r]][:-1]
            else:
                assert sets[0][r] is None and sets[1][r] is None           # never stepped
    # histories of <eos> alone: no frame at all
    only = jctx.plan_priming([np.zeros(0, dtype=np.int64)] * 3, 8)
    assert len(only) == 1 and only[0]["n_steps"] == 0 and only[0]["has"].tolist() == [0, 0, 0] and only[0]["last"].tolist() == [cc.EOS] * 3
    with pytest.raises(ValueError):
        jctx.plan_priming(ctxs, 0)


def test_step_words():
    w, last = jctx.step_words([])
    assert w.tolist() == [] and last == cc.EOS
    w, last = jctx.step_words([4])
    assert w.tolist() == [cc.EOS] and last == 4
    w, last = jctx.step_words([4, cc.EOS, 9])
    assert w.tolist() == [cc.EOS, 4, cc.EOS] and last == 9


# ---------------------------------------------------------------------------------------------- eval split
@pytest.mark.parametrize("words,n,ctx,rest", [
    (["a", "b", "c", "d"], 0, [], ["a", "b", "c", "d"]),
    (["a", "b", "c", "d"], 2, ["a", "b"], ["c", "d"]),
    (["a", "b", "c", "d"], 3, ["a", "b", "c"], ["d"]),
    (["a", "b", "c", "d"], 4, ["a", "b", "c"], ["d"]),              # at least one word is converted
    (["a", "b", "c", "d"], 99, ["a", "b", "c"], ["d"]),
    (["a"], 2, [], ["a"]),                                          # a one-word sentence has no context
    (["a"], 0, [], ["a"]),
])
def test_eval_split(words, n, ctx, rest):
    assert jctx.split_sentence(words, n) == (ctx, rest)


def test_eval_flag_and_log_name():
    from jlm_amd import eval as jeval
    p = jeval.build_parser()
    assert p.parse_args([]).context_words == 0
    assert p.parse_args(["-cw", "3"]).context_words == 3 and p.parse_args(["--context_words", "2"]).context_words == 2
