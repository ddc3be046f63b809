"""The yardstick of the candidate-list tests (tests/test_candidates_cpu.py, tests/test_gpu_candidates.py): the UNMODIFIED oracle.

``context_cases.primed_decode`` gives the oracle's n-best of an input after a left context and leaves the lattice in
``OracleDecoder.backward_lookup``.  The spans of path ``rank`` are read off that lattice, a segment's alternatives are the nodes of
``backward_lookup[start + length]`` with that start and length in list order, and the total of an alternative is the chain rule
(``context_cases.chain_nll``) over the path's ids with the segment's id replaced, out-of-vocabulary words as id 0 -- for a finite
lookahead the substituted chain's terms up to the lookahead and the path's own terms behind it.
"""
import numpy as np

from tests import context_cases as cc

N_CAND = 10
TOPN = 10
SEPARATION = 1e-4          # a position is compared word for word when its yardstick total is further than this from both neighbours
MAX_EXEMPT = 2             # positions per (model, beam) a finite lookahead may leave closer (predict_cases.MAX_EXEMPT)
LOOKAHEADS = (None, 0, 1)
# The positions (input, segment, position) the yardstick alone leaves within SEPARATION of a neighbour, per model: the same for every
# beam and rank that has them, and only with the contexts at lookahead 0 (two alternatives of input 11's first segment whose heads
# differ by less than 1e-4; behind them the path's own terms are added to both).  tests/test_candidates_cpu.py asserts that these are
# ALL of them -- the union over contexts, lookaheads and ranks per (model, beam), at most MAX_EXEMPT -- and the GPU test exempts no other.
EXPECTED_CLOSE = {"vtable": {(11, 0, 3), (11, 0, 4)}}


def inputs():
    """context_cases' 12 ragged inputs and one empty input"""
    return cc.sentences() + [""]


def contexts(V, seed=5):
    """one context per input of :func:`inputs`: context_cases' twelve, and none for the empty input"""
    return cc.contexts(V, seed=seed) + [None]


def spans_of(ends, words):
    """[(start, length)] of the path ``words`` in the lattice ``ends`` (per frame [(start, length, id, word)])"""
    out, start = [], 0
    for w in words:
        lens = {n[1] for f in range(len(ends)) for n in ends[f] if n[0] == start and n[3] == w and f == start + n[1]}
        assert len(lens) == 1, (w, start, lens)
        (ln,) = lens
        out.append((start, ln))
        start += ln
    return out


def alternatives(ends, start, length):
    """the nodes of ``ends[start + length]`` with that start and length, in list order"""
    return [n for n in ends[start + length] if n[0] == start and n[1] == length]


def oracle_terms(o, text, ctx, beam, rank, topN=TOPN):
    """-> (conversions, own, segments): the oracle's n-best, the per-word chain terms of its path ``rank`` (None: no such path) and per
    segment (start, length, [(word, the per-word chain terms of the path with this word in the segment)]) in alternative order"""
    conv = cc.primed_decode(o, text, ctx, topN=topN, beam_width=beam)
    if not len(text) or len(conv) <= rank:
        return conv, None, []
    ends, lm = o.backward_lookup, o.model
    hist = [cc.EOS] + cc.ids_of(ctx)
    words = conv[rank][1]
    ids = cc.path_ids(o, words)
    own = cc.chain_nll(lm, hist, ids)
    segs = []
    for k, (start, ln) in enumerate(spans_of(ends, words)):
        alts = []
        for n in alternatives(ends, start, ln):
            sub = list(ids)
            sub[k] = o.w2i.get(n[3], 0)
            alts.append((n[3], cc.chain_nll(lm, hist, sub)))
        assert any(w == words[k] for w, _t in alts)
        segs.append((start, ln, alts))
    return conv, own, segs


def totals(own, terms, k, lookahead):
    """the total of an alternative of segment k (0-based) from its chain ``terms``: everything up to the lookahead from the substituted
    chain, the path's own terms behind it"""
    K = len(own)
    j = K - 1 - k if lookahead is None else min(K - 1 - k, lookahead)
    return float(terms[:k + 1 + j].sum() + own[k + 1 + j:].sum())


_TERMS, _YARD = {}, {}


def yardstick(name, beam, with_ctx, lookahead=None, rank=0, seed=5):
    """[(conversions, [(start, length, the first N_CAND + 1 candidates (total, word), stably sorted)])] over :func:`inputs`, computed
    once per process; the chains are shared by the lookaheads"""
    key = (name, beam, bool(with_ctx), rank, seed)
    if key not in _TERMS:
        o = cc.oracle(name)
        ctxs = contexts(cc.MODELS[name][0], seed) if with_ctx else [None] * 13
        _TERMS[key] = [oracle_terms(o, text, ctx, beam, rank) for text, ctx in zip(inputs(), ctxs)]
    ykey = key + (lookahead,)
    if ykey not in _YARD:
        out = []
        for conv, own, segs in _TERMS[key]:
            lists = []
            for k, (start, ln, alts) in enumerate(segs):
                t = np.asarray([totals(own, terms, k, lookahead) for _w, terms in alts])
                order = np.argsort(t, kind="stable")[:N_CAND + 1]
                lists.append((start, ln, [(float(t[i]), alts[i][0]) for i in order]))
            out.append((conv, lists))
        _YARD[ykey] = out
    return _YARD[ykey]


def path_terms(name, beam, with_ctx, rank=0, seed=5):
    """[(conversions, own terms, segments)] behind :func:`yardstick` (the self-checks read them)"""
    yardstick(name, beam, with_ctx, None, rank, seed)
    return _TERMS[(name, beam, bool(with_ctx), rank, seed)]


def separated(cands, n_cand=N_CAND):
    """per position < min(n_cand, len): is its total further than SEPARATION from both neighbours (the entry behind the list included)"""
    sc = [c[0] for c in cands[:n_cand + 1]]
    out = []
    for i in range(min(n_cand, len(cands))):
        left = i == 0 or sc[i] - sc[i - 1] > SEPARATION
        right = i + 1 >= len(sc) or sc[i + 1] - sc[i] > SEPARATION
        out.append(left and right)
    return out


def close_positions(name, with_ctx, beam, lookahead, rank=0):
    """the positions of the yardstick's own lists that have a neighbour within SEPARATION: [(input, segment, position)].  None for
    lookahead=None (tests/test_candidates_cpu.py asserts it, and at most MAX_EXEMPT per (model, beam) for a finite lookahead); the
    GPU test exempts exactly these from the word comparison."""
    out = []
    for i, (_conv, lists) in enumerate(yardstick(name, beam, with_ctx, lookahead, rank)):
        for k, (_s, _l, cands) in enumerate(lists):
            out += [(i, k, pos) for pos, ok in enumerate(separated(cands)) if not ok]
    return out


def check_segments(got, want, conv, rank, tag, n_cand=N_CAND):
    """the end-to-end bar for one input: the yardstick's spans and list lengths, sorted scores within the suite's bar (rtol 2e-6 / atol
    2e-5, context_cases.check_nbest's), the same word at every separated position, the own word's score within that bar of
    conversions[rank][0].  -> the positions that were not separated, as (segment, position)"""
    assert [(s, ln) for s, ln, _c in got] == [(s, ln) for s, ln, _c in want], tag
    close = []
    for k, ((_s, _ln, g), (_s2, _ln2, w)) in enumerate(zip(got, want)):
        w10 = w[:n_cand]
        assert len(g) == len(w10), (tag, k, len(g), len(w10))
        gs = [x for x, _ in g]
        assert gs == sorted(gs), (tag, k)
        np.testing.assert_allclose(gs, [x for x, _ in w10], rtol=2e-6, atol=2e-5, err_msg=str((tag, k)))
        for i, ok in enumerate(separated(w, n_cand)):
            if ok:
                assert g[i][1] == w10[i][1], (tag, k, i, g[i], w10[i])
            else:
                close.append((k, i))
        own = [x for x, word in g if word == conv[rank][1][k]]
        if own:                                               # (cut off only where n_cand better alternatives exist)
            np.testing.assert_allclose(min(own, key=lambda x: abs(x - conv[rank][0])), conv[rank][0], rtol=2e-6, atol=2e-5,
                                       err_msg=str((tag, k, "own word")))
        else:
            assert len(g) == n_cand, (tag, k)
    return close
